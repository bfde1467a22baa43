"""The constellation tables (nrLDPC_hip_mod_table, nr_qam.h) against a numpy float32 restatement of the reference's
nr_generate_modulation_table() and the labelling of 38.211 5.1; no GPU."""
import numpy as np
import pytest

from qam_np import mod_table_np


@pytest.fixture(scope="module")
def m():
    import openairinterface5g_amd as hip
    return hip.ldpc


AMPLITUDES = {2: [16384], 4: [7327, 21981], 6: [3575, 10725, 17876, 25026],
              8: [1777, 5331, 8885, 12439, 15993, 19547, 23102, 26656]}


@pytest.mark.parametrize("Qm", [2, 4, 6, 8])
def test_mod_table_equals_the_float32_restatement(m, Qm):
    t = m.mod_table(Qm)
    assert t.shape == (1 << Qm, 2) and t.dtype == np.int16
    assert np.array_equal(t, mod_table_np(Qm))
    assert sorted(set(np.abs(t).reshape(-1).tolist())) == AMPLITUDES[Qm]   # the known answers


@pytest.mark.parametrize("Qm", [2, 4, 6, 8])
def test_labelling_of_38211_5_1(m, Qm):
    """38.211 5.1: re from b(0), b(2), ..., im from b(1), b(3), ...; b(0) / b(1) = 1 is the negative half-plane, and the
    magnitude levels follow the Gray recursion; every point distinct; the mean energy is ~32768^2 / 2 (unit power at 1/sqrt(2) scale)"""
    t = m.mod_table(Qm).astype(np.int64)
    idx = np.arange(1 << Qm)
    assert (np.sign(t[:, 0]) == 1 - 2 * (idx & 1)).all()
    assert (np.sign(t[:, 1]) == 1 - 2 * ((idx >> 1) & 1)).all()
    assert len({(a, b) for a, b in t.tolist()}) == 1 << Qm
    if Qm >= 4:   # b(2) = 0 -> the inner levels of 16QAM (|re| = 1 unit), b(2) = 1 -> the outer (3 units), etc.
        u = AMPLITUDES[Qm][0]
        lev = np.abs(t[:, 0]) // u + (np.abs(t[:, 0]) % u > u // 2)
        n = Qm // 2
        for i in idx:
            L = 1
            for k in range(1, n):
                L = (1 << k) - (1 - 2 * ((i >> (2 * (n - k))) & 1)) * L
            assert abs(lev[i] - L) <= 0, (i, lev[i], L)
    p = (t.astype(np.float64) ** 2).sum(axis=1).mean()
    assert abs(p / (32768.0 ** 2 / 2) - 1.0) < 0.01


@pytest.mark.parametrize("Qm", [0, 1, 3, 5, 7, 9, 10])
def test_bad_qm_is_refused(m, Qm):
    import ctypes as C
    L = m._qam_lib()
    out = np.full(2 * 512, 0x5a5a, np.int16)
    assert L.nrLDPC_hip_mod_table(Qm, out.ctypes.data) == -1
    assert "Qm" in m.last_error()
    assert (out == 0x5a5a).all()
    assert L.nrLDPC_hip_mod_table(4, None) == -1
