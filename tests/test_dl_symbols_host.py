"""Layer mapping and the DL-SCH call to symbols, without a GPU: the numpy layer mapping the GPU tests use against a loop
restatement of the reference's nr_layer_mapping(), and the built library and the header carry both new entry points."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from layer_np import layer_demap_np, layer_map_np

ROOT = Path(__file__).resolve().parent.parent


def nr_layer_mapping_loops(mod_symbs, n_layers, n_symbs):
    """nr_modulation.c:246-270 as loops: mod_symbs[q] = codeword q's points (c16 words) -> tx_layers[l][i].  Cases 1-4 take
    codeword 0 alone; case 6 is restated as the reference writes it (both codewords, three layers each)."""
    if n_layers == 1:
        return [list(mod_symbs[0][:n_symbs])]
    if n_layers <= 4:
        layers = [[None] * (n_symbs // n_layers) for _ in range(n_layers)]
        for i in range(n_symbs // n_layers):
            base = n_layers * i
            for l in range(n_layers):
                layers[l][i] = mod_symbs[0][base + l]
        return layers
    assert n_layers == 6
    layers = [[None] * ((n_symbs + 2) // 3) for _ in range(n_layers)]
    for q in range(2):
        for i in range(0, n_symbs, 3):
            for l in range(3):
                layers[l][i // 3] = mod_symbs[q][i + l]
    return layers


@pytest.mark.parametrize("Nl", [1, 2, 3, 4])
def test_layer_map_np_equals_the_loops(Nl):
    rng = np.random.default_rng(40 + Nl)
    for n in (Nl, 12 * Nl, 1001 * Nl):
        pts = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
        words = pts.view(np.int32).reshape(-1).tolist()
        loops = nr_layer_mapping_loops([words], Nl, n)
        got = layer_map_np(pts, Nl)
        assert got.shape == (Nl, n // Nl, 2)
        assert [got[l].view(np.int32).reshape(-1).tolist() for l in range(Nl)] == loops
        assert np.array_equal(layer_demap_np(got), pts)
    assert np.array_equal(layer_map_np(pts, 1)[0], pts)                  # one layer: the modulation output itself


def test_two_codeword_layers_need_a_second_codeword():
    """Nl = 6 (two codewords in the reference): what lands in the layers depends on mod_symbs[1] -- a second codeword that one
    transport block (one codeword) does not have, hence the refusal of Nl > 4 in nrLDPC_hip_dlsch_encode_symbols"""
    rng = np.random.default_rng(6)
    cw0 = rng.integers(0, 1 << 31, 30).tolist()
    cw1 = rng.integers(0, 1 << 31, 30).tolist()
    cw1b = [x ^ 1 for x in cw1]
    a = nr_layer_mapping_loops([cw0, cw1], 6, 30)
    b = nr_layer_mapping_loops([cw0, cw1b], 6, 30)
    assert a != b                                                        # the second codeword is read
    assert nr_layer_mapping_loops([cw0, cw0], 6, 30)[:3] == [cw0[l::3] for l in range(3)]


def test_library_exports_and_header_declares_the_new_calls(built):
    import openairinterface5g_amd as pkg
    out = subprocess.run(["nm", "-D", "--defined-only", str(pkg.ldpc.LIB_PATH)], capture_output=True, text=True).stdout
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "nrLDPC_hip.h").read_text(), flags=re.S)
    for n in ("nrLDPC_hip_dlsch_encode_symbols", "nrLDPC_hip_layer_mapping"):
        assert re.search(rf"\bT {n}$", out, flags=re.M), n
        assert re.search(rf"^int32_t {n}\(", hdr, flags=re.M), n
        assert n in pkg.ldpc.EXPORTS
    assert re.search(r"nrLDPC_hip_dlsch_encode_symbols\(const nrLDPC_hip_tb_batch_t \*b, const nrLDPC_hip_tb_scr_t \*scr\);", hdr)
    assert re.search(r"nrLDPC_hip_layer_mapping\(const int16_t \*in, uint32_t n_symbs, uint8_t Nl, int16_t \*out, uint32_t "
                     r"layer_stride, int32_t mem,\s+void \*stream\);", hdr)
