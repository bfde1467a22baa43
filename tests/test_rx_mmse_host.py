"""The two-layer MMSE receiver's arithmetic (csrc/nr_rx_mmse.h through nrLDPC_hip_ulsch_mmse_2layers_host / _level_mmse_host, CPU
only) against the numpy restatement of the reference (rx_mmse_np.py), the two numpy formulations against each other, values worked
out by hand, the refusals, and a CPU end-to-end check that fixes the channel the GPU end-to-end test uses (mmse_e2e_case)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as O
from layer_np import symbols_np
from qam_np import demap_np
from rx_mmse_np import level_mmse_lanes, level_mmse_np, mmse_lanes, mmse_np, records_np
from test_scrambling_host import c_init_of
from test_tb_scrambled_emul import unscramble

ROOT = Path(__file__).resolve().parent.parent
M = -32768
NVARS = (0, 1, 37, 70000)          # 70000 = 0x11170 carries into the high half of the packed word
SHIFTS = (0, 3, 9)


def rand_case(rng, n_rx, nb_re, amp=32768):
    return (rng.integers(-amp, amp, (n_rx, nb_re, 2)).astype(np.int16), rng.integers(-amp, amp, (2, n_rx, nb_re, 2)).astype(np.int16))


def corner_case(rng, n_rx, nb_re):
    """full-scale values: every component one of -32768, 32767, 0 or a random value, so that the madd wraps (all four -32768),
    the packs and the adds_epi16 saturate, the add_epi16 of the matched filter wraps and neg16(-32768) stays"""
    pick = lambda shape: np.where(rng.integers(0, 4, shape) == 0, rng.integers(-32768, 32768, shape), rng.choice([M, 32767, M, 0], shape)).astype(np.int16)
    return pick((n_rx, nb_re, 2)), pick((2, n_rx, nb_re, 2))


def host_mmse(m, rx, ch, Qm, s, nvar, pad=0):
    n_rx, nb_re = rx.shape[0], rx.shape[1]
    stride = nb_re + pad
    a, b = np.full((n_rx, stride, 2), 77, np.int16), np.full((2 * n_rx, stride, 2), -77, np.int16)
    a[:, :nb_re], b[:, :nb_re] = rx, ch.reshape(2 * n_rx, nb_re, 2)
    return m.ulsch_mmse_2layers_host(a, b, n_rx, stride, nb_re, Qm, s, nvar)


def test_the_two_numpy_formulations_agree():
    rng = np.random.default_rng(1)
    for n_rx in (2, 4):
        for Qm in (6, 8):
            for nb_re in (12, 18, 30, 5, 100):
                for nvar in NVARS:
                    for s in (SHIFTS if nb_re == 100 else (SHIFTS[(nb_re + nvar + Qm) % 3],)):
                        cases = (rand_case(rng, n_rx, nb_re), corner_case(rng, n_rx, nb_re), rand_case(rng, n_rx, nb_re, 900))
                        for rx, ch in cases[1:2] if nb_re == 100 else cases:
                            assert np.array_equal(mmse_np(rx, ch, Qm, s, nvar), mmse_lanes(rx, ch, Qm, s, nvar)), (n_rx, Qm, nb_re, nvar, s)
    for nb_re in (1, 16, 17, 48, 100):
        for n_rx in (2, 4):
            for max_ch in (0, 2047, 2048, 16384, 32767):
                ch = rand_case(rng, n_rx, nb_re)[1]
                a, b = level_mmse_np(ch, max_ch), level_mmse_lanes(ch, max_ch)
                assert a[0] == b[0] and np.array_equal(a[1], b[1]), (nb_re, n_rx, max_ch)


@pytest.mark.parametrize("n_rx", [2, 4])
@pytest.mark.parametrize("Qm", [6, 8])
def test_mmse_host_equals_numpy(built, n_rx, Qm):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    rng = np.random.default_rng(100 * Qm + n_rx)
    for nb_re in (12, 18, 30, 100):            # 18 and 30: a partial last quad
        for nvar in NVARS:
            for s in SHIFTS:
                for kind, (rx, ch) in enumerate((rand_case(rng, n_rx, nb_re), corner_case(rng, n_rx, nb_re), rand_case(rng, n_rx, nb_re, 900))):
                    got = host_mmse(m, rx, ch, Qm, s, nvar, pad=kind)
                    assert got.shape == (2, Qm // 2, nb_re, 2)
                    assert np.array_equal(got, mmse_np(rx, ch, Qm, s, nvar)), (n_rx, Qm, nb_re, nvar, s, kind)
    # ... and the lane-by-lane restatement: every nb_re, every nvar and every shift (each (nvar, shift) pair at one nb_re at least)
    for i, nb_re in enumerate((12, 18, 30, 100)):
        for k, nvar in enumerate(NVARS):
            for s in (SHIFTS if nb_re == 100 else (SHIFTS[(i + k) % 3],)):
                for rx, ch in (corner_case(rng, n_rx, nb_re), rand_case(rng, n_rx, nb_re, 900)):
                    assert np.array_equal(host_mmse(m, rx, ch, Qm, s, nvar), mmse_lanes(rx, ch, Qm, s, nvar)), (n_rx, Qm, nb_re, nvar, s)
    # a shift outside 0..31 is clamped
    rx, ch = rand_case(rng, n_rx, 21)
    assert np.array_equal(host_mmse(m, rx, ch, Qm, -5, 1), mmse_np(rx, ch, Qm, 0, 1))
    assert np.array_equal(host_mmse(m, rx, ch, Qm, 77, 1), mmse_np(rx, ch, Qm, 31, 1))


def test_hand_computed_values(built):
    """Worked out on paper from :505-548, :646-687, :756-867, :1103-1256, so that the numpy restatement is not the only witness.
    Two antennas, layer 0 seen by antenna 0 alone with h = 16, layer 1 by antenna 1 alone with h = 16j; rx0 = 3 - 2j, rx1 = 5 + j.
    Matched filter: y0 = 16 (3 - 2j) = (48, -32); y1 = conj(16j)(5 + j) = (16, -80).  a = d = (256, 0), b = c = 0."""
    import openairinterface5g_amd as pkg
    m = pkg.ldpc

    def run(nb_re, nvar):
        rx, ch = np.zeros((2, nb_re, 2), np.int16), np.zeros((2, 2, nb_re, 2), np.int16)
        rx[0], rx[1] = (3, -2), (5, 1)
        ch[0, 0], ch[1, 1] = (16, 0), (0, 16)
        got = host_mmse(m, rx, ch, 6, 0, nvar)
        assert np.array_equal(got, mmse_np(rx, ch, 6, 0, nvar)) and np.array_equal(got, mmse_lanes(rx, ch, 6, 0, nvar))
        assert (got == got[:, :, :1]).all()                       # every RE the same
        return got[:, :, 0, :].tolist()

    # det = 65536 in four lanes: sum of det >> 2 = 65536, log2_approx = 17, b = 9; mag = 128; mulhi(128, 20225) = 39 -> 78,
    # mulhi(128, 10112) = 19 -> 38; y0 d = (12288, -8192) >> 9; y1 a = (4096, -20480) >> 9
    assert run(4, 0) == [[[24, -16], [78, 78], [38, 38]], [[8, -40], [78, 78], [38, 38]]]
    # nvar = 0x11170 on the packed word: a = d = (256 + 4464, 0 + 1) = (4720, 1), det = 4720^2 - 1 = 22278399; two REs and two
    # lanes of padding whose a = d = (4464, 1), det = 19927295: sum = 2 * 5569599 + 2 * 4981823 = 21102844, log2_approx = 25, b = 17;
    # mag = 169 -> mulhi 52 -> 104, 26 -> 52; y0 d = (48 * 4720 + 32, -32 * 4720 + 48) = (226592, -150992) >> 17 = (1, -2);
    # y1 a = (16 * 4720 + 80, -80 * 4720 + 16) = (75600, -377584) >> 17 = (0, -3)
    assert run(2, 70000) == [[[1, -2], [104, 104], [52, 52]], [[0, -3], [104, 104], [52, 52]]]


def test_zero_determinant_quad(built):
    """Where the reference aborts (AssertFatal :1181): every lane's det = 0 -> sum 0, log2_approx(0) = 0, b = -8, a left shift by 8
    of zeros: the magnitudes are 0, and y0 d - y1 b = 0 for a rank-one channel (a = b = c = d, y0 = y1)."""
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    rng = np.random.default_rng(5)
    for n_rx in (2, 4):
        rx, ch = rand_case(rng, n_rx, 8, 3000)
        ch[1] = ch[0]
        for Qm in (6, 8):
            got = host_mmse(m, rx, ch, Qm, 4, 0)
            assert not got.any()
            assert not mmse_np(rx, ch, Qm, 4, 0).any() and not mmse_lanes(rx, ch, Qm, 4, 0).any()
    # one singular quad beside a regular one
    rx, ch = rand_case(rng, 2, 8, 3000)
    ch[1, :, :4] = ch[0, :, :4]
    got = host_mmse(m, rx, ch, 6, 4, 0)
    assert not got[:, :, :4].any() and got[:, :, 4:].any() and np.array_equal(got, mmse_lanes(rx, ch, 6, 4, 0))


def test_level_mmse_host_equals_the_transcription(built):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    rng = np.random.default_rng(3)
    seen = set()
    for nb_re in (16, 48, 1, 6 * 51, 100, 3276):
        for n_rx in (2, 4):
            for max_ch in (0, 2047, 2048, 16384, 32767):
                for amp in (32768, 1200):
                    ch = rand_case(rng, n_rx, nb_re, amp)[1]
                    stride = nb_re + int(rng.integers(0, 5))
                    a = np.zeros((2 * n_rx, stride, 2), np.int16)
                    a[:, :nb_re] = ch.reshape(2 * n_rx, nb_re, 2)
                    lv, avg = m.ulsch_level_mmse_host(a, n_rx, stride, nb_re, max_ch)
                    want = level_mmse_lanes(ch, max_ch) if nb_re <= 306 else level_mmse_np(ch, max_ch)
                    assert lv == want[0] and np.array_equal(avg, want[1]), (nb_re, n_rx, max_ch, amp)
                    assert (lv, avg.tolist()) == (level_mmse_np(ch, max_ch)[0], level_mmse_np(ch, max_ch)[1].tolist())
                    seen.add(lv)
    assert len(seen) > 3
    # by hand: 16 REs of (1000, 0) on every pair.  max_ch 1000: shift_ch_ext 0, h' = 1000, avg 1e6, log2_approx 20 -> 10 - 3 = 7;
    # max_ch 16384: shift_ch_ext = log2_approx(8) = 4, ch_amp = 4096, b = 0: h' = 1000 * 4096 >> 16 = 62, 16 terms of 3844 >> 4 = 240, avg 3840, 12 -> 6 - 3 = 3
    ch = np.zeros((4, 16, 2), np.int16)
    ch[:, :, 0] = 1000
    for max_ch, lv_want, avg_want in ((1000, 7, 1000000), (16384, 3, 3840)):
        lv, avg = m.ulsch_level_mmse_host(ch, 2, 16, 16, max_ch)
        assert (lv, avg.tolist()) == (lv_want, [avg_want] * 4)
    assert m.ulsch_level_mmse_host(np.zeros((8, 5, 2), np.int16), 4, 5, 5, 0)[0] == 0


def test_host_checks_refuse_bad_arguments(built):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    z = np.zeros((8, 4, 2), np.int16)
    for bad, why in ((lambda: m.ulsch_mmse_2layers_host(z, z, 1, 4, 4, 6, 0, 0), "n_rx"), (lambda: m.ulsch_mmse_2layers_host(z, z, 3, 4, 4, 6, 0, 0), "n_rx"),
                     (lambda: m.ulsch_mmse_2layers_host(z, z, 8, 4, 4, 6, 0, 0), "n_rx"), (lambda: m.ulsch_mmse_2layers_host(z, z, 2, 4, 4, 4, 0, 0), "Qm"),
                     (lambda: m.ulsch_mmse_2layers_host(z, z, 2, 4, 4, 2, 0, 0), "Qm"), (lambda: m.ulsch_mmse_2layers_host(z, z, 2, 4, 4, 7, 0, 0), "Qm"),
                     (lambda: m.ulsch_level_mmse_host(z, 1, 4, 4, 0), "n_rx"), (lambda: m.ulsch_level_mmse_host(z, 2, 4, 0, 0), "nb_re")):
        with pytest.raises(RuntimeError):
            bad()
        assert why in m.last_error()
    assert set(m.EXPORTS) >= {"nrLDPC_hip_ulsch_channel_level_grid_mmse", "nrLDPC_hip_ulsch_mmse_2layers_grid"}


def test_header_under_the_host_sanitizers(tmp_path):
    """tests/rx_mmse_check.c over the plain-C header, with -fsanitize=address,undefined: no signed overflow, no bad shift"""
    exe = tmp_path / "rx_mmse_check"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    str(ROOT / "openairinterface5g_amd" / "csrc"), "-o", str(exe), str(ROOT / "tests" / "rx_mmse_check.c")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().isdigit(), r.stdout + r.stderr


# ---- end to end on the CPU ------------------------------------------------------------------------------------------------
# The channel of the end-to-end tests, here and on the GPU.  Every path has a gain of 400..480 (c16 units) with a random phase,
# the two layers' columns nearly orthogonal (well conditioned): |h|^2 lies in [2^17, 2^18), so log2_approx(avgs) = 18
# and log2_maxh = 9 - 3 = 6 with max_ch < 2048 (shift_ch_ext = 0).  Then a = d = sum |h|^2 >> 6 is about 3000 n_rx: the matched
# filter's int16 sum (a + |b|) * 1.53 (the largest 64QAM / 256QAM point, in units of the mean amplitude) stays below 32768 for
# n_rx = 4, and det = a d is about 3.6e7 (n_rx = 2) / 1.4e8 (n_rx = 4), shifted to 128..255 by b: the constellation's levels are
# 2 * 190 / sqrt(42) = 58 (64QAM) or 2 * 190 / sqrt(170) = 29 (256QAM) units apart.  A louder channel saturates a and d (adds_epi16),
# a fainter one loses the levels.  Noise: sigma = 3 per component on a received amplitude of about 600, nvar = 2 sigma^2 = 18.
E2E_GAIN, E2E_SIGMA, E2E_NVAR, E2E_RB = (400, 480), 3.0, 18, 4


def mmse_e2e_case(Qm, n_rx):
    """(tb, scrambling, payload, per-symbol nb_re, H int16 [2, n_rx, 2], max_ch, seed for the noise): one two-layer block of 4
    RBs, 13 symbols with 12 REs per RB and a type-1 DMRS symbol with 6"""
    from test_gpu_tb_chain import valid_tbs
    rng = np.random.default_rng(4000 + 10 * Qm + n_rx)
    syms = [12 * E2E_RB] * 2 + [6 * E2E_RB] + [12 * E2E_RB] * 11
    G = Qm * 2 * sum(syms)
    tb = dict(A=valid_tbs(G // 3, 2), G=G, BG=2, Qm=Qm, Nl=2, rv=0, tbslbrm=0)
    scr = (int(rng.integers(0, 0x10000)), 0, int(rng.integers(0, 1024)))
    pay = rng.integers(0, 256, tb["A"] // 8, dtype=np.uint8)
    # antenna a has a gain g_a and a phase of its own; layer 1's column is layer 0's turned by one angle and with every other
    # antenna's sign flipped: orthogonal but for the spread of the gains
    g, ph, th = rng.uniform(*E2E_GAIN, n_rx), rng.uniform(0, 2 * np.pi, n_rx), rng.uniform(0, 2 * np.pi)
    col = g * np.exp(1j * ph)
    hc = np.stack([col, col * np.exp(1j * th) * (-1.0) ** np.arange(n_rx)])                   # [layer, antenna]
    H = np.rint(np.stack([hc.real, hc.imag], -1)).astype(np.int16)
    return tb, scr, pay, syms, np.ascontiguousarray(H), int(np.abs(H).max()), 7000 + Qm + n_rx


def mmse_e2e_channel(planes, H, seed):
    """y_a = sum_l H[l, a] x_l / 23170 + n; planes = int16 [2, R, 2] (the layers' points).  Returns rx int16 [n_rx, R, 2] and the
    estimates int16 [2, n_rx, R, 2] (flat: H at every RE)."""
    rng = np.random.default_rng(seed)
    R, n_rx = planes.shape[1], H.shape[1]
    x = (planes[..., 0].astype(np.float64) + 1j * planes[..., 1]) / 23170.0
    hq = H[..., 0].astype(np.float64) + 1j * H[..., 1]
    y = np.einsum("la,lr->ar", hq, x) + E2E_SIGMA * (rng.standard_normal((n_rx, R)) + 1j * rng.standard_normal((n_rx, R)))
    rx = np.clip(np.rint(np.stack([y.real, y.imag], 2)), -32768, 32767).astype(np.int16)
    return rx, np.ascontiguousarray(np.broadcast_to(H[:, :, None, :], (2, n_rx, R, 2)))


def mmse_e2e_record(tb, syms, rx, ch, lv, receiver=mmse_np):
    """the block's symbol record (flat int16, G entries) out of the numpy receiver, symbol by symbol"""
    Qm, plane = tb["Qm"], tb["G"] // tb["Qm"]
    rec, off = np.zeros(tb["G"], np.int16), 0
    for nb in syms:
        records_np(rec, receiver(rx[:, off:off + nb], ch[:, :, off:off + nb], Qm, lv, E2E_NVAR), Qm, plane, off)
        off += nb
    return rec


@pytest.mark.parametrize("Qm,n_rx", [(6, 2), (6, 4), (8, 2), (8, 4)])
def test_cpu_end_to_end_reference_arithmetic_decodes(built, Qm, n_rx):
    tb, scr, pay, syms, H, max_ch, seed = mmse_e2e_case(Qm, n_rx)
    assert max_ch < 2048
    bits = O.dlsch_encode(tb, pay)
    planes = symbols_np(bits, scr, Qm, 2)
    rx, ch = mmse_e2e_channel(planes, H, seed)
    lv = level_mmse_np(ch[:, :, :syms[0]], max_ch)[0]
    assert lv == 6
    rec = mmse_e2e_record(tb, syms, rx, ch, lv)
    plane = tb["G"] // Qm
    pl = rec.reshape(Qm // 2, plane, 2)
    llr = demap_np(pl[0], list(pl[1:]), Qm)                       # the record is in codeword order: the layers are de-mapped
    llr = unscramble(llr, c_init_of(*scr), 0)
    s = O.segmentation(None, O.len_with_crc(1, tb["A"]), tb["BG"])
    harq = [np.zeros(66 * 384 + 16, np.int16) for _ in range(s["C"])]
    got, ack, iters, _ = O.ulsch_decode(tb, llr, harq, 8)
    assert ack and np.array_equal(got, pay), (Qm, n_rx, iters)
