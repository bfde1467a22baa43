"""Inputs shared by tests/test_dec_block_ends_emul.py and tests/test_gpu_dec_block_ends.py: per code, LLR rows picked by the oracle's
own pass count -- one that stops with pass count 3, one with 4 and one that runs to the cap (numMaxIter 8, reported as 9) -- with the
oracle's output rows.  Computed once per code and process."""
import functools

import numpy as np

import oracle_lib as O
from common import make_llr

CAP = 8
# BG1 / BG2 at Zc = 8: ncore Z = 208 / 112 bits, no multiple of 64; Zc = 12 and 20: output words straddle columns, ncore Z = 312 no
# multiple of 32; Zc = 64: a column is two words; Zc = 384: the lifting size's own instantiation, at R = 1/3 (504 zero words behind
# ncore Z) and 8/9.  Every one-block fast kernel's prologue and hard decision run at each of them
CODES = [(1, 8, 13), (2, 8, 15), (1, 12, 13), (2, 20, 15), (1, 64, 13), (1, 384, 13), (1, 384, 89)]
WANTED = (3, 4, CAP + 1)


@functools.lru_cache(maxsize=None)
def stop_rows(BG, Z, R):
    """(llr int8[3, ncols Z], n_iter int32[3], out uint8[3, out_bytes]) with n_iter = WANTED, by the oracle."""
    rng = np.random.default_rng(77000 + 100 * Z + 10 * BG + R)
    n = O.NCOLS[(BG, R)] * Z
    found = {}
    # from hopeless to easy and round again: small codes need many draws for an exact pass count, large ones a narrow SNR window
    for k in range(4000):
        if len(found) == len(WANTED):
            break
        snr = -12.0 if CAP + 1 not in found else -3.0 + (k % 48) * 0.25
        llr = np.ascontiguousarray(make_llr(rng, BG, Z, R, snr)[:n], np.int8)
        it, out = O.decode(BG, Z, R, llr, CAP)
        if it in WANTED and it not in found:
            found[it] = (llr, out.copy())
    assert len(found) == len(WANTED), (BG, Z, R, sorted(found))
    llr = np.stack([found[w][0] for w in WANTED])
    out = np.stack([found[w][1] for w in WANTED])
    llr.setflags(write=False)
    out.setflags(write=False)
    return llr, np.array(WANTED, np.int32), out
