"""numpy restatements for the modulation / demapping tests: the reference's constellation tables (openair1/PHY/NR_REFSIG/
nr_gen_mod_table.c:35-94, float32 products left to right, truncated into int16), nr_modulation() by definition (symbol i =
bits iQm .. iQm+Qm-1) and the per-RE demapper of nr_ulsch_compute_llr() (abs = _mm_abs_epi16, subs = saturating)."""
import numpy as np

F32 = np.float32
SCALE = {2: F32(0.70711), 4: F32(0.31623), 6: F32(0.15430), 8: F32(0.076696)}


def mod_table_np(Qm):
    """int16[2^Qm, 2] as nr_generate_modulation_table() writes its table of Qm"""
    val, sqrt2, s = F32(32768.0), F32(0.70711), SCALE[Qm]
    out = np.zeros((1 << Qm, 2), np.int16)
    for i in range(1 << Qm):
        for ax in (0, 1):
            b = [(i >> (ax + 2 * k)) & 1 for k in range(Qm // 2)]
            if Qm == 2:
                lev = 1 - 2 * b[0]
            elif Qm == 4:
                lev = (1 - 2 * b[0]) * (2 - (1 - 2 * b[1]))
            elif Qm == 6:
                lev = (1 - 2 * b[0]) * (4 - (1 - 2 * b[1]) * (2 - (1 - 2 * b[2])))
            else:
                lev = (1 - 2 * b[0]) * (8 - (1 - 2 * b[1]) * (4 - (1 - 2 * b[2]) * (2 - (1 - 2 * b[3]))))
            v = F32(F32(F32(F32(lev) * val) * s) * sqrt2)
            out[i, ax] = np.int16(np.trunc(v))
    return out


def bits_of_words(words, length):
    w = np.asarray(words, np.uint32)
    return ((w[:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)[:length].astype(np.uint8)


def modulate_np(words, length, Qm):
    """int16[length/Qm, 2]: point of bits iQm .. iQm+Qm-1 (bit b = index bit b)"""
    b = bits_of_words(words, length).reshape(-1, Qm).astype(np.int64)
    idx = (b << np.arange(Qm)).sum(axis=1)
    return mod_table_np(Qm)[idx]


def _abs16(x):
    x = x.astype(np.int32)
    return np.where(x == -32768, -32768, np.abs(x))


def _subs16(a, b):
    return np.clip(a.astype(np.int32) - b.astype(np.int32), -32768, 32767)


def demap_np(y, mags, Qm):
    """int16[nb_re * Qm]: y, mags = int16 [nb_re, 2] arrays (re, im)"""
    y = np.asarray(y, np.int16).reshape(-1, 2)
    if Qm == 2:
        return (y.astype(np.int32) >> 3).astype(np.int16).reshape(-1)
    lv = [y.astype(np.int32)]
    for m in mags[:Qm // 2 - 1]:
        lv.append(_subs16(np.asarray(m, np.int16).reshape(-1, 2), _abs16(lv[-1])))
    return np.stack(lv, axis=1).astype(np.int16).reshape(-1)


def edge_symbols(rng, nb_re, Qm, amp=20000):
    """y and Qm/2 - 1 magnitude planes (int16 [nb_re, 2]) with -32768 in y and at every intermediate level, magnitudes 0 and
    32767, and values that saturate"""
    y = rng.integers(-amp, amp, (nb_re, 2)).astype(np.int16)
    mags = [rng.integers(0, 32768, (nb_re, 2)).astype(np.int16) for _ in range(Qm // 2 - 1)]
    k = min(nb_re, 16)
    y[:k:4] = -32768                                               # A = -32768: abs stays -32768, B saturates
    y[1:k:4] = 32767
    if mags:
        mags[0][:k] = [[0, 32767]]
        mags[0][2:k:4] = 0
        y[2:k:4] = [[-32767, 32767]]                                # B = 0 - 32767 = -32767 ...
        mags[0][3:k:4] = [[-32768 + 1, 0]]                          # ... and a magnitude that makes B = -32768 exactly
        y[3:k:4] = [[1, 0]]
    if len(mags) > 1:
        mags[1][2:k:4] = [[32767, 0]]                               # C = subs(32767, |-32767|) = 0 / subs(0, ...)
        mags[1][3:k:4] = [[0, 32767]]                               # |B| = |-32768| = -32768: C = subs(0, -32768) saturates
    if len(mags) > 2:
        mags[2][:k] = [[32767, 0]]
    return y, mags
