"""numpy restatement of the reference's nr_layer_mapping() for one codeword (openair1/PHY/MODULATION/nr_modulation.c:246-270):
layer l of the Nl layers takes the codeword's symbols l, l + Nl, l + 2 Nl, ...; and the symbol output of
nrLDPC_hip_dlsch_encode_symbols by its definition (scrambling, nr_modulation, layer mapping)."""
import numpy as np

from qam_np import modulate_np
from test_scrambling_host import c_init_of, serial_gold, words_of


def layer_map_np(points, Nl):
    """int16[n, 2] (c16 points in codeword order) -> int16[Nl, n / Nl, 2]: plane l entry i = point Nl i + l"""
    p = np.asarray(points, np.int16).reshape(-1, 2)
    assert p.shape[0] % Nl == 0
    return np.ascontiguousarray(p.reshape(-1, Nl, 2).transpose(1, 0, 2))


def layer_demap_np(planes):
    """the inverse: int16[Nl, n / Nl, 2] -> int16[n, 2] in codeword order"""
    p = np.asarray(planes, np.int16)
    return np.ascontiguousarray(p.transpose(1, 0, 2)).reshape(-1, 2)


def symbols_np(bits, scrambling, Qm, Nl):
    """the layer planes of one codeword: G bits (one per byte) -> scrambled with (n_rnti, q, n_id) -> points -> Nl planes"""
    G = bits.size
    b = np.zeros((G + 31) // 32 * 32, np.uint8)
    b[:G] = (np.asarray(bits) & 1) ^ serial_gold(c_init_of(*scrambling), G)
    return layer_map_np(modulate_np(words_of(b), G, Qm), Nl)
