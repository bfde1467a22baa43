"""CPU emulation of de-matching with the symbol source (tests/emul/tb_rx_sym_emul.cpp: tb_rx_core.h reading a symbol record,
a workgroup's threads walked phase by phase) against numpy demapping, then numpy unscrambling, then the oracle's
de-interleaving, rate de-matching and pack.  No GPU."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as O
import softbuf_np as SB
from qam_np import demap_np, edge_symbols
from test_tb_scrambled_emul import unscramble

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openairinterface5g_amd" / "csrc"
CXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    d = tmp_path_factory.mktemp("sym_emul")
    subprocess.run(["gcc", "-O2", "-fPIC", "-c", str(CSRC / "nr_coding_host.c"), "-o", str(d / "nr_coding_host.o")], check=True)
    lib = d / "libtb_rx_sym_emul.so"
    subprocess.run([CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-Wno-pass-failed", "-o", str(lib),
                    str(ROOT / "tests" / "emul" / "tb_rx_sym_emul.cpp"), str(d / "nr_coding_host.o")], check=True)
    L = C.CDLL(str(lib))
    L.tb_emul_rx_dematch_sym.argtypes = [C.c_uint32, C.c_int] + [C.c_uint32] * 4 + [C.c_int] + [C.c_uint32] * 3 + \
        [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


def test_demapper_edge_values_numpy_is_the_definition():
    """the numpy demapper on hand-made values (the definition the emulation is checked against)"""
    y = np.array([[-32768, 32767], [-8, 7]], np.int16)
    ma = np.array([[0, 0], [100, -5]], np.int16)
    mb = np.array([[32767, -32768], [0, 0]], np.int16)
    llr = demap_np(y, [ma, mb], 6).reshape(2, 6)
    # RE 0: A = (-32768, 32767); |A| = (-32768, 32767); B = subs(0, -32768) = 32767, subs(0, 32767) = -32767
    #       C = subs(32767, 32767) = 0, subs(-32768, 32767) = -32768
    assert llr[0].tolist() == [-32768, 32767, 32767, -32767, 0, -32768]
    assert llr[1].tolist() == [-8, 7, 92, -12, -92, -12]
    assert demap_np(y, [], 2).tolist() == [-4096, 4095, -1, 0]


def test_rx_dematch_phases_symbol_source_against_the_oracle(emul):
    rng = np.random.default_rng(3303)
    cases = chunked = laps = 0
    for BG, A, lbrm in ((1, 30000, 0), (1, 30000, 24000), (2, 3000, 0), (2, 640, 0), (1, 100000, 150000)):
        s = O.segmentation(None, O.len_with_crc(1, A), BG)
        Z, K, F, Cn = s["Z"], s["K"], s["F"], s["C"]
        N = (66 if BG == 1 else 50) * Z
        for Qm in (2, 4, 6, 8):
            for rv in (0, 2):
                for rate in (0.6, 0.92, 0.08):                       # 0.08: E > Ncb, several laps (and several chunks)
                    E = max(Qm * 4, int((K - F) / rate) // Qm * Qm)
                    R, _ = O.get_R(rv, E, BG, Z, 0, 0)
                    ncols = O.NCOLS[(BG, R)]
                    # the block's record: this segment's symbols behind `pre` symbols of earlier segments, and `post` after
                    pre, post = int(rng.integers(0, 300)), int(rng.integers(0, 40))
                    S = pre + E // Qm + post
                    y, mags = edge_symbols(rng, S, Qm, amp=int(rng.choice([300, 20000])))
                    rec = np.concatenate([y.reshape(-1)] + [m_.reshape(-1) for m_ in mags]).astype(np.int16)
                    assert rec.size == S * Qm
                    bit_off = pre * Qm
                    f = demap_np(y, mags, Qm)[bit_off:bit_off + E]
                    c_init = int(rng.integers(0, 1 << 31))
                    for clear in (1, 0):
                        w0 = rng.integers(-2000, 2000, 66 * 384 + 16).astype(np.int16)
                        Ncb = N if not lbrm else min(N, (3 * lbrm // (2 * Cn)))
                        e = O.deinterleave(E, Qm, unscramble(f, c_init, bit_off))
                        d_ref = w0[:N].copy()                    # dirty behind Ncb too: R0 on round 0, as it is otherwise
                        if clear:
                            SB.clear_segment(d_ref, Ncb, BG, Z, R)
                        rc, d_ref = O.rate_match_rx(lbrm, BG, Z, d_ref, e, Cn, rv, clear, E, F, K - F - 2 * Z)
                        assert rc == 0
                        l_ref = O.llr_prepack(d_ref, BG, Z, K, F, ncols)
                        w = w0.copy()
                        l = np.full(ncols * Z + 8, 0x11, np.int8)
                        rec_in = rec.copy()
                        span = emul.tb_emul_rx_dematch_sym(lbrm, BG, Z, Cn, F, K, rv, E, Qm, ncols * Z, clear, 256, c_init, bit_off,
                                                           rec_in.ctypes.data, 2 * S, w.ctypes.data, l.ctypes.data)
                        assert span > 0
                        key = (BG, A, Qm, rv, rate, clear, bit_off)
                        assert np.array_equal(rec_in, rec), key                 # the record is only read
                        assert np.array_equal(w[:N], d_ref), key
                        assert np.array_equal(w[N:], w0[N:]), key
                        assert np.array_equal(l[:ncols * Z], l_ref), key
                        assert (l[ncols * Z:] == 0x11).all()
                        cases += 1
                        chunked += E // Qm > (512 - 2) * 32 // Qm
                        laps += E > Ncb
    assert cases > 200 and chunked > 10 and laps > 10


def test_rx_dematch_symbol_source_at_the_sequence_chunk_edges(emul):
    """segments of exactly c - 1, c, c + 1 and 2c symbols (c = the symbols of one staged sequence chunk, in which the
    symbols are also demapped) for every Qm, behind an odd number of earlier symbols and behind a word-aligned one, rv 0
    and 3, a plain and an LBRM code: against numpy demapping, unscrambling and the oracle"""
    from test_tb_scrambled_emul import scr_chunk
    rng = np.random.default_rng(4080)
    hit = {}
    for BG, A, lbrm in ((1, 30000, 0), (2, 3000, 0), (1, 30000, 24000)):
        s = O.segmentation(None, O.len_with_crc(1, A), BG)
        Z, K, F, Cn = s["Z"], s["K"], s["F"], s["C"]
        N = (66 if BG == 1 else 50) * Z
        Ncb = N if not lbrm else min(N, (3 * lbrm // (2 * Cn)))
        for Qm in (2, 4, 6, 8):
            c = scr_chunk(Qm)
            for edge, EQ in (("c-1", c - 1), ("c", c), ("c+1", c + 1), ("2c", 2 * c)):
                for rv, odd in ((0, True), (3, False), (3, True)):
                    E = EQ * Qm
                    R, _ = O.get_R(rv, E, BG, Z, 0, 0)
                    ncols = O.NCOLS[(BG, R)]
                    pre = int(rng.integers(0, 150)) * 2 + 1 if odd else int(rng.integers(0, 10)) * 32
                    assert (pre * Qm % 32 != 0) == odd
                    S = pre + EQ + int(rng.integers(0, 40))
                    y, mags = edge_symbols(rng, S, Qm, amp=int(rng.choice([300, 20000])))
                    rec = np.concatenate([y.reshape(-1)] + [m_.reshape(-1) for m_ in mags]).astype(np.int16)
                    bit_off = pre * Qm
                    f = demap_np(y, mags, Qm)[bit_off:bit_off + E]
                    c_init = int(rng.integers(0, 1 << 31))
                    for clear in (1, 0):
                        w0 = rng.integers(-2000, 2000, 66 * 384 + 16).astype(np.int16)
                        e = O.deinterleave(E, Qm, unscramble(f, c_init, bit_off))
                        d_ref = w0[:N].copy()
                        if clear:
                            SB.clear_segment(d_ref, Ncb, BG, Z, R)
                        rc, d_ref = O.rate_match_rx(lbrm, BG, Z, d_ref, e, Cn, rv, clear, E, F, K - F - 2 * Z)
                        assert rc == 0
                        l_ref = O.llr_prepack(d_ref, BG, Z, K, F, ncols)
                        w = w0.copy()
                        l = np.full(ncols * Z + 8, 0x11, np.int8)
                        rec_in = rec.copy()
                        span = emul.tb_emul_rx_dematch_sym(lbrm, BG, Z, Cn, F, K, rv, E, Qm, ncols * Z, clear, 256, c_init, bit_off,
                                                           rec_in.ctypes.data, 2 * S, w.ctypes.data, l.ctypes.data)
                        assert span > 0
                        key = (BG, A, Qm, rv, edge, clear, bit_off)
                        assert np.array_equal(rec_in, rec), key
                        assert np.array_equal(w[:N], d_ref), key
                        assert np.array_equal(w[N:], w0[N:]), key
                        assert np.array_equal(l[:ncols * Z], l_ref), key
                        assert (l[ncols * Z:] == 0x11).all()
                    hit[(Qm, edge, odd)] = hit.get((Qm, edge, odd), 0) + 1
    assert len(hit) == 4 * 4 * 2 and min(hit.values()) >= 3
