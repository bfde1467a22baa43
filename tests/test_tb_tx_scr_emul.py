"""CPU emulation of the fused TX kernel's packed, scrambled store (tests/emul/tb_tx_scr_emul.cpp: tb_tx_scr.h, the code the
GPU runs, and the library's own plan of the words segments share) against its definition: the oracle chain's coded bits XOR
the bit-serial Gold sequence, 32 to a word, zeros behind G.  Segments and their selection chunks run in many orders, with
small chunks to multiply the chunk boundaries.  No GPU."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as O
from test_scrambling_host import serial_gold, words_of

ROOT = Path(__file__).resolve().parent.parent
CXX = "/opt/rocm/lib/llvm/bin/clang++"
GUARD = 8
SENT = 0x5A5A5A5A


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    d = tmp_path_factory.mktemp("tx_scr_emul")
    lib = d / "libtb_tx_scr_emul.so"
    subprocess.run([CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", str(lib),
                    str(ROOT / "tests" / "emul" / "tb_tx_scr_emul.cpp")], check=True)
    L = C.CDLL(str(lib))
    L.tb_emul_tx_scr.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p,
                                 C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    return L


def want_words(bits, c_init):
    G = bits.size
    x = bits ^ serial_gold(c_init, G)
    return words_of(np.concatenate([x, np.zeros(-G % 32, np.uint8)]))


def orders(rng, nch):
    """step lists: segments in order, reversed, two seeded permutations, and chunks of all segments round-robin"""
    n = len(nch)
    seq = lambda perm: np.concatenate([np.full(nch[q], q, np.uint32) for q in perm])
    out = [seq(range(n)), seq(range(n - 1, -1, -1)), seq(rng.permutation(n)), seq(rng.permutation(n))]
    rr, left = [], list(nch)
    perm = rng.permutation(n)
    while any(left):
        for q in perm:
            if left[q]:
                rr.append(q)
                left[q] -= 1
    out.append(np.array(rr, np.uint32))
    return out


def geometry(Es, Qm, chunk):
    """what the store will meet, from the same E / bit_off arithmetic as the plan: per segment the shared words and the
    chunk carries (a chunk boundary inside a word)"""
    cnt = dict(head=0, tail=0, carry=0, carry_and_ticket=0, last_mid=0, ch1=0, ch2=0, ch3=0)
    lo = 0
    for r, E in enumerate(Es):
        hi, last = lo + E, r + 1 == len(Es)
        head = lo % 32 != 0
        tail = not last and hi % 32 != 0 and not (head and (hi - 1) // 32 == lo // 32)
        nch = -(-(E // Qm) // chunk)
        carry = any((lo + k * chunk * Qm) % 32 for k in range(1, nch))
        cnt["head"] += head
        cnt["tail"] += tail
        cnt["carry"] += carry
        cnt["carry_and_ticket"] += carry and (head or tail)
        cnt["last_mid"] += last and hi % 32 != 0
        cnt["ch1" if nch == 1 else "ch2" if nch == 2 else "ch3"] += 1
        lo = hi
    return cnt


def tb_cases():
    """(tb, E list or None = the chain's nr_get_E split): every Qm, Nl 1..4, rv 0..3, LBRM, repetition (E > Ncb)"""
    out = []
    for Qm in (2, 4, 6, 8):
        for BG, A, Nl, rv, lbrm, rate, extra in ((1, 20000, 1, 0, 0, 0.6, 1), (2, 3000, 3, 2, 0, 0.3, 0), (2, 4008, 2, 1, 0, 0.5, 1),
                                                  (1, 30000, 2, 3, 24000, 0.7, 1), (1, 20000, 4, 1, 0, 0.12, 1),
                                                  (1, 9000, 3, 0, 0, 0.9, 2)):
            unit = Qm * Nl
            G = (int(A / rate) // unit + extra) * unit               # extra: G / unit not a multiple of C -> two E sizes
            out.append((dict(A=A, G=G, BG=BG, Qm=Qm, Nl=Nl, rv=rv, tbslbrm=lbrm), None))
    return out


def run(emul, bits, Es, Qm, c_init, chunk, steps, tickets, parts, nt, rng):
    G = bits.size
    nw = (G + 31) // 32
    out = np.full(nw + 2 * GUARD, SENT, np.uint32)
    out[GUARD:GUARD + nw] = rng.integers(0, 1 << 32, nw, dtype=np.uint64).astype(np.uint32)  # every word must be stored
    E_arr = np.asarray(Es, np.uint32)
    plan = np.zeros(2, np.uint32)
    rc = emul.tb_emul_tx_scr(len(Es), E_arr.ctypes.data, Qm, c_init, bits.ctypes.data, chunk, nt, steps.ctypes.data, steps.size,
                             out[GUARD:].ctypes.data, tickets.ctypes.data, tickets.size, parts.ctypes.data, parts.size,
                             plan.ctypes.data)
    assert rc == 0
    assert (out[:GUARD] == SENT).all() and (out[GUARD + nw:] == SENT).all()   # nothing outside the block's words
    assert (tickets == 0).all()                                              # every ticket zero again for the next call
    return out[GUARD:GUARD + nw], plan


def test_packed_scrambled_store_against_the_oracle(emul):
    rng = np.random.default_rng(4711)
    tot = dict(head=0, tail=0, carry=0, carry_and_ticket=0, last_mid=0, ch1=0, ch2=0, ch3=0)
    runs = three_part_words = 0
    seen = set()
    cases = tb_cases()
    # segments split by hand, some shorter than a word (the chain's contract, E >= K - F - 2Zc, never makes one; the store
    # and the plan must still settle a word that three segments share): bits of a real codeword, cut anew
    for Qm in (2, 4, 6):
        cases.append((dict(A=4008, G=Qm * 2000, BG=2, Qm=Qm, Nl=1, rv=0, tbslbrm=0),
                      [Qm * e for e in (5, 3, 1, 700, 7, 2, 1, 9, 11, 1000, 1, 4, 256)]))
    for t, split in cases:
        Qm, G = t["Qm"], t["G"]
        pay = rng.integers(0, 256, t["A"] // 8, dtype=np.uint8)
        bits = np.ascontiguousarray(O.dlsch_encode(t, pay))
        assert bits.size == G
        Cn = O.segmentation(None, O.len_with_crc(1, t["A"]), t["BG"])["C"]
        Es = [O.get_E(G, Cn, Qm, t["Nl"], r) for r in range(Cn)] if split is None else split
        assert sum(Es) == G
        if split is not None:
            assert min(Es) < 32 and sum(Es) == G
        c_init = int(rng.integers(0, 1 << 31))
        want = want_words(bits, c_init)
        tickets = np.zeros(2 * len(Es) + 1, np.uint32)
        parts = rng.integers(0, 1 << 32, 2 * len(Es) + 1, dtype=np.uint64).astype(np.uint32)   # parts need no clearing
        for chunk in (2048, 96, 64, 32):
            nch = [-(-(E // Qm) // chunk) for E in Es]
            g = geometry(Es, Qm, chunk)
            for k in tot:
                tot[k] += g[k]
            for o, steps in enumerate(orders(rng, nch)):
                got, plan = run(emul, bits, Es, Qm, c_init, chunk, steps, tickets, parts, 64 if o % 2 else 7, rng)
                assert np.array_equal(got, want), (t, Es[:4], chunk, o, int(np.flatnonzero(got != want)[0]))
                three_part_words += int(plan[1]) > 2 * int(plan[0])
                runs += 1
        seen.add((Qm, t["Nl"], t["rv"], bool(t["tbslbrm"]), max(Es) > 66 * 384))
    print("tx scr emulation:", runs, "runs,", tot, "three-part words:", three_part_words)
    # (the sweep as it stands: 540 runs; head 248, tail 196, carry 125, both 125, last mid-word 84, 1/2/3+ chunks 159/10/227)
    assert runs >= 500
    assert tot["head"] >= 200 and tot["tail"] >= 150 and tot["carry"] >= 100 and tot["carry_and_ticket"] >= 100
    assert tot["last_mid"] >= 60 and tot["ch1"] >= 100 and tot["ch2"] >= 8 and tot["ch3"] >= 150
    assert three_part_words >= 40                                           # words that three segments share
    assert {s[0] for s in seen} == {2, 4, 6, 8} and {s[1] for s in seen} == {1, 2, 3, 4} and {s[2] for s in seen} == {0, 1, 2, 3}
    assert any(s[3] for s in seen) and any(s[4] for s in seen)             # LBRM; repetition (E > N of the largest code)


def test_bad_step_lists_are_refused(emul):
    bits = np.zeros(256, np.uint8)
    Es = np.array([128, 128], np.uint32)
    tickets, parts, plan = np.zeros(8, np.uint32), np.zeros(8, np.uint32), np.zeros(2, np.uint32)
    out = np.zeros(16, np.uint32)
    call = lambda steps, chunk=32, Qm=2: emul.tb_emul_tx_scr(2, Es.ctypes.data, Qm, 1, bits.ctypes.data, chunk, 8, steps.ctypes.data,
                                                               steps.size, out.ctypes.data, tickets.ctypes.data, 8, parts.ctypes.data, 8,
                                                               plan.ctypes.data)
    assert call(np.array([0, 0, 1, 1], np.uint32)) == 0
    assert call(np.array([0, 0, 1], np.uint32)) == -2                       # a segment not run to its end
    assert call(np.array([0, 0, 0, 1, 1], np.uint32)) == -2                 # a chunk too many
    assert call(np.array([0, 0, 1, 1], np.uint32), chunk=48) == -1          # chunk % 32
    assert call(np.array([0, 0, 1, 1], np.uint32), Qm=3) == -1
