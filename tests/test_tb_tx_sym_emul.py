"""CPU emulation of the fused TX kernel's symbol store (tests/emul/tb_tx_sym_emul.cpp: tb_tx_sym.h, the code the GPU runs, on
one segment's selection chunks) against its definition: numpy Gold scrambling, then modulate_np, then layer_map_np.  No GPU."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from layer_np import symbols_np

ROOT = Path(__file__).resolve().parent.parent
CXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    d = tmp_path_factory.mktemp("tx_sym_emul")
    lib = d / "libtb_tx_sym_emul.so"
    subprocess.run([CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", str(lib),
                    str(ROOT / "tests" / "emul" / "tb_tx_sym_emul.cpp")], check=True)
    L = C.CDLL(str(lib))
    L.tb_emul_tx_sym.argtypes = [C.c_void_p] + [C.c_uint32] * 7 + [C.c_int, C.c_void_p]
    return L


def split_E(rng, G, Qm, Nl, n_seg):
    """segment lengths as nr_hip_get_E cuts a codeword (multiples of Qm Nl), with a random number of segments"""
    unit = Qm * Nl
    units = G // unit
    cuts = np.sort(rng.choice(np.arange(1, units), n_seg - 1, replace=False)) if n_seg > 1 else np.array([], int)
    bounds = [0] + [int(c) for c in cuts] + [units]
    return [(bounds[k + 1] - bounds[k]) * unit for k in range(n_seg)]


@pytest.mark.parametrize("Qm", [2, 4, 6, 8])
@pytest.mark.parametrize("Nl", [1, 2, 3, 4])
def test_symbol_store_against_numpy(emul, Qm, Nl):
    rng = np.random.default_rng(17 * Qm + Nl)
    odd_starts = chunk_off = 0
    for S_units, n_seg, chunk in ((7, 1, 2048), (1000, 3, 2048), (3000, 2, 2048), (800, 5, 96), (1, 1, 32)):
        G = S_units * Qm * Nl * (3 if chunk == 2048 and S_units > 100 else 1)
        bits = rng.integers(0, 2, G).astype(np.uint8)
        scr = (int(rng.integers(0, 0x10000)), int(rng.integers(0, 2)), int(rng.integers(0, 1024)))
        want = symbols_np(bits, scr, Qm, Nl)
        S = G // Qm
        rec = np.full(S + 8, 0x5a5a5a5a, np.uint32)
        c_init = (scr[0] << 15) + (scr[1] << 14) + scr[2]
        bit_off = 0
        for E in split_E(rng, G, Qm, Nl, min(n_seg, G // (Qm * Nl))):
            f = np.ascontiguousarray(bits[bit_off:bit_off + E])
            assert emul.tb_emul_tx_sym(f.ctypes.data, E, Qm, Nl, S // Nl, c_init, bit_off, chunk, 64, rec.ctypes.data) == 0
            odd_starts += bit_off % 32 != 0
            # a chunk after the first starts at codeword symbol bit_off / Qm + k chunk: not a layer boundary when Nl does not divide it
            chunk_off += any((bit_off // Qm + k * chunk) % Nl for k in range(1, (E // Qm + chunk - 1) // chunk))
            bit_off += E
        assert np.array_equal(rec[:S].view(np.int16).reshape(Nl, S // Nl, 2), want), (Qm, Nl, G, chunk)
        assert (rec[S:] == 0x5a5a5a5a).all()                             # nothing behind the record
    assert Qm == 8 or odd_starts > 0                                     # segments that start inside a sequence word
    assert Nl in (1, 2, 4) or chunk_off > 0                              # Nl = 3: chunks that start inside a layer group


def test_bad_arguments_are_refused(emul):
    f = np.zeros(64, np.uint8)
    rec = np.zeros(64, np.uint32)
    assert emul.tb_emul_tx_sym(f.ctypes.data, 36, 6, 5, 1, 1, 0, 2048, 64, rec.ctypes.data) == -1   # Nl = 5
    assert emul.tb_emul_tx_sym(f.ctypes.data, 30, 6, 2, 1, 1, 0, 2048, 64, rec.ctypes.data) == -1   # E % (Qm Nl)
    assert emul.tb_emul_tx_sym(f.ctypes.data, 36, 6, 2, 1, 1, 0, 100, 64, rec.ctypes.data) == -1    # chunk % 32
