"""-m gpu: the four scrambled / symbol chain calls (nrLDPC_hip_dlsch_encode_scrambled, _dlsch_encode_symbols,
_ulsch_decode_scrambled, _ulsch_decode_symbols) against references that never go through the library: the oracle chain
(oracle_lib), bit-serial Gold scrambling, and the numpy mapper, demapper and layer mapping.  The shapes sit on the kernels'
chunk edges, derived from the constants: segments of TB_TX_SEL_SYMS symbols around the fused TX kernel's selection chunk,
segments around the fused RX kernel's sequence chunk of (TB_RX_SCR_WORDS - 2) 32 / Qm symbols, the largest codeword the
calls accept (2^21 bits) and the refusal just above it; then four HARQ rounds per memory mode and seeded random sweeps."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as O
from layer_np import symbols_np
from qam_np import demap_np
from test_gpu_qam import rx_symbols
from test_gpu_tb_chain import valid_tbs
from test_scrambling_host import c_init_of, serial_gold, words_of
from test_tb_scrambled_emul import unscramble

pytestmark = pytest.mark.gpu
CSRC = Path(__file__).resolve().parent.parent / "openairinterface5g_amd" / "csrc"
SEL = int(re.search(r"#define TB_TX_SEL_SYMS (\d+)", (CSRC / "tb_chain.h").read_text()).group(1))
SCR_WORDS = int(re.search(r"#define TB_RX_SCR_WORDS (\d+)u", (CSRC / "tb_jobs.h").read_text()).group(1))
MAX_G = 1 << 21                                                       # NR_SCR_MAX_BITS


def rx_chunk(Qm):
    return (SCR_WORDS - 2) * 32 // Qm


def geom(t):
    """the chain's segment geometry (tb_api.inc.cpp): C, Foffset = K - F - 2Zc, per segment E and codeword bit_off"""
    s = O.segmentation(None, O.len_with_crc(1, t["A"]), t["BG"])
    Es = [O.get_E(t["G"], s["C"], t["Qm"], t["Nl"], r) for r in range(s["C"])]
    return s["C"], s["K"] - s["F"] - 2 * s["Z"], Es, list(np.cumsum([0] + Es[:-1]))


def fits(t):
    """the rate-matching contract of the library and of the reference: E >= K - F - 2Zc for every segment"""
    _, fo, Es, _ = geom(t)
    return min(Es) >= fo


def tb_at(Qm, Nl, C_want, EQs_total, rv=0, A_list=(4008, 8000, 12000, 20000, 30000)):
    """a transport block of C_want segments whose G is EQs_total symbols: the first base graph and A (of A_list) that
    segment into C_want blocks and fit the contract; None when none does"""
    for BG in (2, 1):
        for a in A_list:
            A = valid_tbs(a, BG)
            if O.segmentation(None, O.len_with_crc(1, A), BG)["C"] != C_want:
                continue
            t = dict(A=A, G=EQs_total * Qm, BG=BG, Qm=Qm, Nl=Nl, rv=rv, tbslbrm=0)
            if fits(t):
                return t
    return None


def scr_bits(t, pay, scr):
    bits = O.dlsch_encode(t, pay)
    return bits, bits ^ serial_gold(c_init_of(*scr), t["G"])


def rand_scr(rng):
    return (int(rng.integers(0, 0x10000)), int(rng.integers(0, 2)), int(rng.integers(0, 1024)))


# ---- encode ---------------------------------------------------------------------------------------------------------------
def check_encode(m, tbs, rng):
    """both encode calls on one heterogeneous batch against the oracle; sentinels around every block untouched"""
    scr = [rand_scr(rng) for _ in tbs]
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
    words = m.dlsch_encode_scrambled_host(tbs, pays, scr)
    planes = m.dlsch_encode_symbols_host(tbs, pays, scr)
    for t, p, s, w, pl in zip(tbs, pays, scr, words, planes):
        bits, x = scr_bits(t, p, s)
        want = words_of(np.concatenate([x, np.zeros(-t["G"] % 32, np.uint8)]))
        assert w.size == want.size and np.array_equal(w, want), (t, s, int(np.flatnonzero(w != want)[0]))
        assert np.array_equal(pl, symbols_np(bits, s, t["Qm"], t["Nl"])), (t, s)
    # sentinels: the host wrappers place the blocks in one array with 16-byte spacing; run once more into a poisoned array
    co, total = m.tb_layout_packed(tbs)
    L = m._tb_lib()
    po = np.cumsum([0] + [(t["A"] // 8 + 15) // 16 * 16 for t in tbs])
    pay = np.zeros(int(po[-1]) + 16, np.uint8)
    for i, p in enumerate(pays):
        pay[po[i]:po[i] + p.size] = p
    out = np.full(total // 4 + 8, 0xA5A5A5A5, np.uint32)
    arr = m._tb_array(tbs, po, co, None)
    b = m.nrLDPC_hip_tb_batch_t(n_tb=len(tbs), tb=arr, payload=pay.ctypes.data, coded=out.ctypes.data, harq=None, harq_stride=0,
                                ack=None, iter_max=None, mem=m.MEM_HOST, stream=None)
    assert L.nrLDPC_hip_dlsch_encode_scrambled(C.byref(b), m._scr_array(scr, len(tbs))) == 0
    mask = np.ones(out.size, bool)
    for i, (t, w) in enumerate(zip(tbs, words)):
        n = (t["G"] + 31) // 32
        assert np.array_equal(out[co[i] // 4:co[i] // 4 + n], w)
        mask[co[i] // 4:co[i] // 4 + n] = False
    assert (out[mask] == 0xA5A5A5A5).all()
    cs, total_s = m.tb_layout_symbols(tbs)
    out = np.full(total_s // 4 + 8, 0xA5A5A5A5, np.uint32)
    arr = m._tb_array(tbs, po, cs, None)
    b = m.nrLDPC_hip_tb_batch_t(n_tb=len(tbs), tb=arr, payload=pay.ctypes.data, coded=out.ctypes.data, harq=None, harq_stride=0,
                                ack=None, iter_max=None, mem=m.MEM_HOST, stream=None)
    assert L.nrLDPC_hip_dlsch_encode_symbols(C.byref(b), m._scr_array(scr, len(tbs))) == 0
    mask = np.ones(out.size, bool)
    for i, (t, pl) in enumerate(zip(tbs, planes)):
        n = t["G"] // t["Qm"]
        assert np.array_equal(out[cs[i] // 4:cs[i] // 4 + n].view(np.int16).reshape(pl.shape), pl)
        mask[cs[i] // 4:cs[i] // 4 + n] = False
    assert (out[mask] == 0xA5A5A5A5).all()


def tx_edge_tbs():
    """per Qm, segments of EQ in {S-1, S, S+1, 2S, 2S+1} (S = TB_TX_SEL_SYMS) rounded to the layers; G that gives the two E
    sizes (a segment boundary inside a word); Nl = 3, where a layer group straddles a chunk"""
    tbs = []
    for Qm in (2, 4, 6, 8):
        for e in (SEL - 1, SEL, SEL + 1, 2 * SEL, 2 * SEL + 1):
            for Nl, Cw, extra in ((1, 2, 0), (1, 3, 1), (3, 2, 1), (2, 4, 1)):
                eq = e // Nl * Nl
                t = tb_at(Qm, Nl, Cw, Cw * eq + extra * Nl, rv=(e + Nl) % 4)
                if t is not None:
                    tbs.append(t)
    return tbs


def test_encode_calls_at_the_selection_chunk_edges(hip):
    rng = np.random.default_rng(2048)
    tbs = tx_edge_tbs()
    hits, mid = {}, 0
    for t in tbs:
        _, _, Es, offs = geom(t)
        for E, o in zip(Es, offs):
            hits[(t["Qm"], E // t["Qm"])] = hits.get((t["Qm"], E // t["Qm"]), 0) + 1
            mid += o % 32 != 0
    for Qm in (2, 4, 6, 8):                                            # every edge exactly, for every Qm (Nl = 1)
        for e in (SEL - 1, SEL, SEL + 1, 2 * SEL, 2 * SEL + 1):
            assert hits.get((Qm, e), 0) >= 2, (Qm, e)
    assert mid >= 20 and sum(t["Nl"] == 3 for t in tbs) >= 15
    print("tx edges:", len(tbs), "blocks,", sum(hits.values()), "segments,", mid, "starting inside a word")
    check_encode(hip.ldpc, tbs, rng)


# ---- decode ---------------------------------------------------------------------------------------------------------------
def rx_inputs(rng, t, x, sigma):
    """scrambled LLRs of the scrambled bits x, and the symbol record of their points; both with -32768 / 32767 among them"""
    G = t["G"]
    llr = np.clip(np.round((1 - 2 * x.astype(np.float64)) * 8 + sigma * rng.standard_normal(G)), -200, 200).astype(np.int16)
    k = rng.integers(0, G, 6)
    llr[k[:3]] = np.where(x[k[:3]], -32768, 32767)                     # saturated, right sign ...
    llr[k[3:]] = [-32768, 32767, -32768]                               # ... and anything
    y, mags = rx_symbols(rng, words_of(np.concatenate([x, np.zeros(-G % 32, np.uint8)])), G, t["Qm"], sigma / 40.0)
    return llr, y, mags


class Decoder:
    """both decode calls and their references over HARQ rounds, in one memory mode"""

    def __init__(self, m, tbs, mode, ids0):
        self.m, self.tbs, self.mode = m, tbs, mode
        self.segs = [geom(t)[0] for t in tbs]
        n = len(tbs)
        self.ids = {k: [ids0 + 1000 * j + i for i in range(n)] for j, k in enumerate(("scr", "sym"))}
        self.harq = {k: np.zeros((sum(self.segs), m.HARQ_STRIDE), np.int16) for k in ("scr", "sym")}
        self.ref = {k: [[np.zeros(m.HARQ_STRIDE, np.int16) for _ in range(c)] for c in self.segs] for k in ("scr", "sym")}
        self.state = {k: [0] * n for k in ("scr", "sym")}
        self.llrlen = {k: [0] * n for k in ("scr", "sym")}

    def call(self, kind, rx, inputs, scr):
        import torch
        m = self.m
        fn_host = m.ulsch_decode_scrambled_host if kind == "scr" else m.ulsch_decode_symbols_host
        if self.mode == "host":
            return fn_host(rx, inputs, self.harq[kind], scr)
        if self.mode == "harq_library":
            return fn_host(rx, inputs, None, scr, harq_ids=self.ids[kind])
        po, co, ho, _ = m.tb_layout(rx)                                 # "device": every buffer on the GPU
        src = torch.zeros(int(co[-1]) + 16, dtype=torch.int16)
        for i, v in enumerate(inputs):
            src[co[i]:co[i] + v.size] = torch.from_numpy(v)
        src = src.cuda()
        h = torch.from_numpy(self.harq[kind].reshape(-1)).cuda()
        pay = torch.zeros(int(po[-1]) + 16, dtype=torch.uint8, device="cuda")
        ack = torch.zeros(len(rx), dtype=torch.uint8, device="cuda")
        itm = torch.zeros(len(rx), dtype=torch.int32, device="cuda")
        (m.ulsch_decode_scrambled_device if kind == "scr" else m.ulsch_decode_symbols_device)(rx, src, h, pay, ack, itm, scrambling=scr)
        torch.cuda.synchronize()
        self.harq[kind][:] = h.cpu().numpy().reshape(self.harq[kind].shape)
        ph = pay.cpu().numpy()
        return [ph[po[i]:po[i] + t["A"] // 8] for i, t in enumerate(rx)], ack.cpu().numpy().astype(bool), itm.cpu().numpy()

    def round(self, rnd, rv, pays, scr, rng, sigmas):
        """one round (rv) of every block through both calls; everything compared with the oracle.  Returns the ACKs"""
        m = self.m
        cur = [dict(t) if rv is None else dict(t, rv=rv) for t in self.tbs]
        llrs, recs, ref_llr = [], [], {"scr": [], "sym": []}
        for t, p, s, sg in zip(cur, pays, scr, sigmas):
            _, x = scr_bits(t, p, s)
            llr, y, mags = rx_inputs(rng, t, x, sg)
            llrs.append(llr)
            recs.append(m.pack_symbol_records([[y] + mags])[0])
            ref_llr["scr"].append(unscramble(llr, c_init_of(*s), 0))
            ref_llr["sym"].append(unscramble(demap_np(y, mags, t["Qm"]), c_init_of(*s), 0))
        acks = {}
        for kind, inputs in (("scr", llrs), ("sym", recs)):
            rx = [dict(t, round=rnd, llrLen=self.llrlen[kind][i]) for i, t in enumerate(cur)]
            keep = [v.copy() for v in inputs]
            out, ack, itm = self.call(kind, rx, inputs, scr)
            assert all(np.array_equal(a, b) for a, b in zip(keep, inputs))            # the inputs are only read
            row = 0
            for i, t in enumerate(cur):
                p_ref, ack_ref, its, self.state[kind][i] = O.ulsch_decode(t, ref_llr[kind][i], self.ref[kind][i], 8, rnd,
                                                                          self.state[kind][i], vec=True)
                key = (kind, self.mode, rnd, rv, i, t["A"], t["G"], t["Qm"], t["Nl"])
                assert bool(ack[i]) == ack_ref and itm[i] == max(its), key + (its, int(itm[i]))
                assert rx[i]["llrLen"] == self.state[kind][i], key
                if ack_ref:
                    assert np.array_equal(out[i], p_ref), key
                if self.mode == "harq_library":
                    got = m.harq_read(self.ids[kind][i], self.segs[i] * m.HARQ_STRIDE).reshape(self.segs[i], -1)
                else:
                    got = self.harq[kind][row:row + self.segs[i]]
                for r in range(self.segs[i]):
                    assert np.array_equal(got[r], self.ref[kind][i][r]), key + (r,)
                row += self.segs[i]
                self.llrlen[kind][i] = rx[i]["llrLen"]
            acks[kind] = ack
        return acks

    def release(self):
        if self.mode == "harq_library":
            for k in ("scr", "sym"):
                for i in self.ids[k]:
                    self.m.harq_release(i)


def rx_edge_tbs():
    """per Qm, segments of EQ in {c-1, c, c+1, 2c, 2c+1} (c = the RX sequence chunk); with C = 3 the later segments start
    inside a word"""
    tbs = []
    for Qm in (2, 4, 6, 8):
        c = rx_chunk(Qm)
        for i, e in enumerate((c - 1, c, c + 1, 2 * c, 2 * c + 1)):
            for Cw, extra in ((2, 0), (3, 2)):
                t = tb_at(Qm, 1, Cw, Cw * e + extra, rv=(0, 2, 3, 1, 0)[i])
                if t is not None:
                    tbs.append(t)
    return tbs


def test_decode_calls_at_the_sequence_chunk_edges(hip):
    rng = np.random.default_rng(8160)
    tbs = rx_edge_tbs()
    hits, odd = {}, 0
    for t in tbs:
        _, _, Es, offs = geom(t)
        for E, o in zip(Es, offs):
            hits[(t["Qm"], E // t["Qm"])] = hits.get((t["Qm"], E // t["Qm"]), 0) + 1
            odd += o % 32 != 0
    for Qm in (2, 4, 6, 8):
        c = rx_chunk(Qm)
        for e in (c - 1, c, c + 1, 2 * c, 2 * c + 1):
            assert hits.get((Qm, e), 0) >= 2, (Qm, e)
    assert odd >= 10
    print("rx edges:", len(tbs), "blocks,", sum(hits.values()), "segments,", odd, "starting inside a word")
    d = Decoder(hip.ldpc, tbs, "host", 0)
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
    acks = d.round(0, None, pays, [rand_scr(rng) for _ in tbs], rng, [4.0] * len(tbs))
    assert acks["scr"].sum() >= len(tbs) // 2


# ---- the largest codeword, and the refusal above it -----------------------------------------------------------------------
def big_tb():
    return dict(A=valid_tbs(600000, 1), G=MAX_G, BG=1, Qm=8, Nl=4, rv=0, tbslbrm=0)


def test_largest_codeword_through_all_four_calls(hip):
    rng = np.random.default_rng(21)
    t = big_tb()
    Cn, _, Es, offs = geom(t)
    assert fits(t) and sum(Es) == MAX_G and offs[-1] // 32 > 60000      # the last segments jump ~65 000 words in
    check_encode(hip.ldpc, [t], rng)
    d = Decoder(hip.ldpc, [t], "host", 0)
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8)]
    acks = d.round(0, 0, pays, [rand_scr(rng)], rng, [3.0])
    assert acks["scr"].all() and acks["sym"].all()
    print("G = 2^21:", Cn, "segments, last at word", offs[-1] // 32)


def test_codeword_above_the_largest_is_refused_before_any_work(hip):
    m = hip.ldpc
    L = m._tb_lib()
    t = dict(big_tb(), G=MAX_G + 8 * 4, round=0)
    pay = np.zeros(t["A"] // 8 + 16, np.uint8)
    scr = m._scr_array([(1, 0, 1)], 1)
    out = np.full(MAX_G // 8 + 64, 0xA5A5A5A5, np.uint32)
    for fn in (L.nrLDPC_hip_dlsch_encode_scrambled, L.nrLDPC_hip_dlsch_encode_symbols):
        arr = m._tb_array([t], [0], [0], None)
        b = m.nrLDPC_hip_tb_batch_t(n_tb=1, tb=arr, payload=pay.ctypes.data, coded=out.ctypes.data, harq=None, harq_stride=0, ack=None,
                                    iter_max=None, mem=m.MEM_HOST, stream=None)
        assert fn(C.byref(b), scr) < 0 and "2^21" in m.last_error()
        assert (out == 0xA5A5A5A5).all()
    segs = geom(t)[0]
    llr = np.ones(t["G"] + 16, np.int16)
    harq = np.full((segs, m.HARQ_STRIDE), 7, np.int16)
    for fn in (L.nrLDPC_hip_ulsch_decode_scrambled, L.nrLDPC_hip_ulsch_decode_symbols):
        ack, itm = np.full(1, 9, np.uint8), np.full(1, 9, np.int32)
        arr = m._tb_array([t], [0], [0], [0])
        b = m.nrLDPC_hip_tb_batch_t(n_tb=1, tb=arr, payload=pay.ctypes.data, coded=llr.ctypes.data, harq=harq.ctypes.data,
                                    harq_stride=m.HARQ_STRIDE, ack=ack.ctypes.data, iter_max=itm.ctypes.data, mem=m.MEM_HOST, stream=None)
        assert fn(C.byref(b), scr) < 0 and "2^21" in m.last_error()
        assert (harq == 7).all() and ack[0] == 9 and itm[0] == 9 and (pay == 0).all() and (llr == 1).all()


# ---- HARQ: four rounds per memory mode ------------------------------------------------------------------------------------
def harq_tbs():
    mk = lambda a, G, BG, Qm, Nl, lbrm=0: dict(A=valid_tbs(a, BG), G=G // (Qm * Nl) * Qm * Nl, BG=BG, Qm=Qm, Nl=Nl, rv=0, tbslbrm=lbrm)
    return [mk(20000, 30000, 1, 6, 3), mk(64000, 96000, 1, 8, 4), mk(5000, 14400, 2, 2, 1), mk(30000, 48000, 1, 4, 2, lbrm=24000),
            mk(9000, 16320, 1, 2, 1), mk(3000, 9600, 2, 4, 3)]


@pytest.mark.parametrize("mode", ["host", "device", "harq_library"])
def test_four_harq_rounds_against_the_oracle(hip, mode):
    rng = np.random.default_rng({"host": 1, "device": 2, "harq_library": 3}[mode])
    tbs = harq_tbs()
    assert all(fits(t) for t in tbs)
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
    scr = [rand_scr(rng) for _ in tbs]
    d = Decoder(hip.ldpc, tbs, mode, 7000)
    # noise that leaves most blocks NACKed until round 2 or 3
    first_ack = [None] * len(tbs)
    try:
        for rnd, rv in enumerate((0, 2, 3, 1)):
            acks = d.round(rnd, rv, pays, scr, rng, [9.0, 9.0, 9.0, 9.0, 9.0, 6.0])
            for i, a in enumerate(acks["scr"]):
                if a and first_ack[i] is None:
                    first_ack[i] = rnd
    finally:
        d.release()
    print(mode, "first ACK round per block:", first_ack)
    assert sum(r is not None and r >= 2 for r in first_ack) >= 1          # some block only decodes in round 3 or 4


# ---- random sweeps --------------------------------------------------------------------------------------------------------
def random_tbs(rng, n, max_bits, decodable):
    tbs = []
    while len(tbs) < n:
        bits = int(np.exp(rng.uniform(np.log(24), np.log(max_bits))))
        BG = 2 if bits <= 292 else (int(rng.integers(1, 3)) if bits <= 30000 else 1)
        Qm, Nl = int(rng.choice([2, 4, 6, 8])), int(rng.integers(1, 5))
        A = valid_tbs(bits, BG)
        rate = rng.uniform(0.15, 0.95 if not decodable else 0.8)
        G = max(1, int(A / rate) // (Qm * Nl)) * Qm * Nl
        t = dict(A=A, G=G, BG=BG, Qm=Qm, Nl=Nl, rv=int(rng.integers(0, 4)), tbslbrm=int(rng.choice([0, 0, 2 * A, 3 * A])))
        if G <= MAX_G and fits(t):                                      # (E >= Foffset: the contract)
            tbs.append(t)
    return tbs


def test_encode_calls_random_sweep(hip):
    rng = np.random.default_rng(20261016)
    tbs = random_tbs(rng, 32, 120000, False)
    assert {t["Nl"] for t in tbs} == {1, 2, 3, 4} and {t["Qm"] for t in tbs} == {2, 4, 6, 8}
    check_encode(hip.ldpc, tbs, rng)


def test_decode_calls_random_sweep(hip):
    rng = np.random.default_rng(20261017)
    tbs = random_tbs(rng, 32, 120000, True)
    assert {t["Nl"] for t in tbs} >= {3, 4} and any(t["A"] >= 60000 for t in tbs)
    d = Decoder(hip.ldpc, tbs, "host", 0)
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
    acks = d.round(0, None, pays, [rand_scr(rng) for _ in tbs], rng, list(rng.choice([3.0, 5.0, 9.0], len(tbs))))
    assert acks["scr"].sum() >= 8
