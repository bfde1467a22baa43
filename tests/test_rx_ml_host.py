"""The two-layer max-log ML receiver's arithmetic (csrc/nr_rx_ml.h through nrLDPC_hip_ulsch_ml_2layers_host / _level_ml_host, CPU
only) against the numpy restatement of the reference (rx_ml_np.py), the two numpy formulations against each other on the REs the
reference's loop covers, values worked out by hand, the refusals, and a CPU end-to-end check that fixes the channel the GPU
end-to-end test uses (ml_e2e_case)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as O
import rx_ml_np as R
from layer_np import symbols_np
from rx_ml_np import level_ml_np, llr_np, ml_lanes, ml_np, rho_lanes, rho_np
from rx_mmse_np import level_mmse_lanes
from test_rx_mmse_host import corner_case, mmse_e2e_case, mmse_e2e_channel, rand_case
from test_scrambling_host import c_init_of
from test_tb_scrambled_emul import unscramble

ROOT = Path(__file__).resolve().parent.parent
SHIFTS = (0, 3, 9)
# nb_re -> (REs of the segment the reference's loop computes, REs behind nb_re it stores): `for (i = 0; i < nb_re >> 3; i += 2)`,
# 16 REs per pass
COVER = {18: (16, 0), 36: (32, 0), 12: (12, 4), 24: (24, 8), 16: (16, 0), 48: (48, 0), 5: (0, 0)}


def host_ml(m, rx, ch, Qm, s, pad=0):
    n_rx, nb_re = rx.shape[0], rx.shape[1]
    stride = nb_re + pad
    a, b = np.full((n_rx, stride, 2), 77, np.int16), np.full((2 * n_rx, stride, 2), -77, np.int16)
    a[:, :nb_re], b[:, :nb_re] = rx, ch.reshape(2 * n_rx, nb_re, 2)
    return m.ulsch_ml_2layers_host(a, b, n_rx, stride, nb_re, Qm, s)


@pytest.mark.parametrize("Qm", [2, 4])
def test_the_two_numpy_formulations_agree_where_the_reference_computes(Qm):
    """... and which REs those are: an uncomputed tail (18, 36), an overrun (12, 24), exact (16, 48), nothing at all (5)"""
    rng = np.random.default_rng(10 + Qm)
    for nb_re, (n_cov, n_over) in COVER.items():
        for n_rx in (2, 4, 3):
            for k, (rx, ch) in enumerate((rand_case(rng, n_rx, nb_re), corner_case(rng, n_rx, nb_re), rand_case(rng, n_rx, nb_re, 900))):
                s = SHIFTS[(k + n_rx) % 3]
                per_re = ml_np(rx, ch, Qm, s)
                for mem_offset in ((0, 1, 3) if Qm == 2 and n_rx == 2 else (0,)):
                    llr, stored, shifted = ml_lanes(rx, ch, Qm, s, mem_offset)
                    assert stored[:nb_re].tolist() == [1] * n_cov + [0] * (nb_re - n_cov), (nb_re, stored)
                    assert stored[nb_re:].tolist() == [1] * n_over + [0] * (len(stored) - nb_re - n_over), (nb_re, stored)
                    L = llr.reshape(2, -1, Qm)
                    assert not L[:, n_cov + n_over:].any()                 # whatever the buffer held: here zeros
                    if Qm == 4:
                        assert not shifted.any()
                        ok = np.arange(n_cov)
                    else:
                        # nr_ulsch_shift_llr: REs 0 .. mem_offset + 4 (nb_re >> 2) - 1 once, the rest never; the same range of the
                        # next symbol then shifts this one's overrun again
                        n_sh = mem_offset + 4 * (nb_re >> 2)
                        assert shifted.tolist() == [1] * n_sh + [0] * (len(shifted) - n_sh)
                        ok = np.arange(min(n_cov, n_sh))
                        never = np.arange(min(n_cov, n_sh), n_cov)         # computed and stored, but left unshifted
                        for l in range(2):
                            assert np.array_equal(L[l, never] >> 4, per_re[never, l])
                    for l in range(2):
                        assert np.array_equal(L[l, ok], per_re[ok, l]), (Qm, nb_re, n_rx, k, l)
    assert COVER[18][0] < 18 and COVER[36][0] < 36 and COVER[12][1] == 4 and COVER[24][1] == 8


@pytest.mark.parametrize("n_rx", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("Qm", [2, 4])
def test_ml_host_equals_numpy_on_every_re(built, n_rx, Qm):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    rng = np.random.default_rng(100 * Qm + n_rx)
    for nb_re in (12, 18, 36, 16, 1, 100):
        for s in SHIFTS:
            for kind, (rx, ch) in enumerate((rand_case(rng, n_rx, nb_re), corner_case(rng, n_rx, nb_re), rand_case(rng, n_rx, nb_re, 900))):
                got = host_ml(m, rx, ch, Qm, s, pad=kind)
                assert got.shape == (nb_re, 2, Qm)
                assert np.array_equal(got, ml_np(rx, ch, Qm, s)), (n_rx, Qm, nb_re, s, kind)
    # a shift outside 0..31 is clamped
    rx, ch = rand_case(rng, n_rx, 21)
    assert np.array_equal(host_ml(m, rx, ch, Qm, -5), ml_np(rx, ch, Qm, 0))
    assert np.array_equal(host_ml(m, rx, ch, Qm, 77), ml_np(rx, ch, Qm, 31))


def test_full_scale_inputs_saturate_every_kind_of_instruction(built):
    """the streams, magnitudes and rho at full scale straight into the two LLR functions, and full-scale estimates into rho: the
    saturating adds and subs clamp in both functions, packs_epi32 and adds_epi16 clamp in rho -- and the C code follows"""
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    rng = np.random.default_rng(77)
    pick = lambda n: rng.choice(np.array([-32768, 32767, -32768, 0, 12345, -23456], np.int64), n)
    n = 4000
    for fn, args in ((R.qpsk_qpsk_lanes, 6), (R.qam16_qam16_lanes, 8)):
        R.SATURATED.update(adds=0, subs=0)
        out = fn(*[pick(n) for _ in range(args)])
        assert R.SATURATED["adds"] > n and R.SATURATED["subs"] > n, (fn.__name__, R.SATURATED)
        assert all((-32768 <= v).all() and (v <= 32767).all() for v in out)
        assert any((v == 32767).any() for v in out) and any((v == -32768).any() for v in out)
    for Qm in (2, 4):
        for n_rx in (2, 4):
            rx, ch = corner_case(rng, n_rx, 64)
            R.SATURATED.update(adds=0, subs=0)
            rho = rho_np(ch, 0)
            assert R.SATURATED == dict(adds=0, subs=0)                       # rho_np clamps with _sat16 itself
            assert any((np.abs(r) >= 32767).any() for r in rho)
            p = ch.astype(np.int64)
            assert (np.abs(p[0, 0, :, 0] * p[1, 0, :, 0] + p[0, 0, :, 1] * p[1, 0, :, 1]) > 32767).any()   # packs_epi32 clamps
            R.SATURATED.update(adds=0, subs=0)
            want = ml_np(rx, ch, Qm, 0)
            assert R.SATURATED["adds"] > 0 and R.SATURATED["subs"] > 0
            assert np.array_equal(host_ml(m, rx, ch, Qm, 0), want)


def test_hand_computed_values(built):
    """Worked out on paper from :505-571 and the two LLR functions, so that the numpy restatement is not the only witness.  Two
    antennas, layer 0 seen by antenna 0 alone, layer 1 by antenna 1 alone: rho = 0, every |psi| is |y1| (QPSK: / 2)."""
    import openairinterface5g_amd as pkg
    m = pkg.ldpc

    def run(Qm, h, rx0, rx1, nb_re=3):
        rx, ch = np.zeros((2, nb_re, 2), np.int16), np.zeros((2, 2, nb_re, 2), np.int16)
        rx[0], rx[1] = rx0, rx1
        ch[0, 0], ch[1, 1] = (h, 0), (0, h)
        got = host_ml(m, rx, ch, Qm, 0)
        assert np.array_equal(got, ml_np(rx, ch, Qm, 0)) and (got == got[:1]).all()
        return got[0].tolist()

    # QPSK, h = 16: y0 = 16 (3 - 2j) = (48, -32), y1 = conj(16j) (5 + j) = (16, -80).
    # layer 0: y0/sqrt2 = 2 mulhi((48, -32), 23170) = (32, -24); y1/2 = (8, -40): |psi_r| = 8, |psi_i| = 40 everywhere.
    #   num_re_p = 48 + 32 - 24 = 56, num_re_m = 48 + 32 + 24 = 104, den_re_p = 48 - 32 - 24 = -8, den_re_m = 48 - 32 + 24 = 40
    #   L1 = max(56, 104) - max(-8, 40) = 64, L2 = max(56, -8) - max(104, 40) = -48; >> 4: 4, -3
    # layer 1: y0 = (16, -80) -> (10, -58); y1/2 = (24, -16): sum 40.  num_re_p = -8, num_re_m = 108, den_re_p = -28, den_re_m = 88
    #   L1 = 108 - 88 = 20, L2 = -8 - 108 = -116; >> 4: 1, -8
    assert run(2, 16, (3, -2), (5, 1)) == [[4, -3], [1, -8]]
    # 16QAM, h = 64: |h|^2 = 4096, mag = mulhrs(4096, 20724) = 2591 for both layers; y0 = (1920, -1280), y1 = -64j (50 + 10j) =
    # (640, -3200).  Layer 0: psi_r = 640 < 2591 -> a_r = 10362; psi_i = 3200 -> a_i = 31086; psi_a = 2 * 101 + 2 * 1517 = 3236;
    # a_sq = 204 + 1842 = 2046 (10362: 1638 -> 3276, 1294 -> 2588, 102 -> 204; 31086: 14745 -> 29490, 11656 -> 23312, 921 -> 1842);
    # y0/sqrt10 = (607, -405), 3 y0/sqrt10 = (1820, -1216): y0_s = 202, -609, 1415, 604, 1012, 1823, 2225, 3036; the channel terms
    # 409, 2048, 2048, 3684.  Bit metrics 0..7: 983, -1467, 557, -1890, 1793, 965, 1367, 542; 8..15: -231, -2681, -3083, -5530, 579,
    # -249, -2273, -3098.  L = 1793 - 579, 983 - 1793, 1793 - 1367, 1793 - 965.
    assert run(4, 64, (30, -20), (50, 10))[0] == [1214, -810, 426, 828]


def test_rho01_and_rho10_are_formed_separately(built):
    """h0 = 3, h1 = j, shift 1: conj(h0) h1 = 3j -> (0, 1); conj(h1) h0 = -3j -> (0, -2), not the conjugate (0, -1)"""
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    ch = np.zeros((2, 1, 16, 2), np.int16)
    ch[0, 0], ch[1, 0] = (3, 0), (0, 1)
    r01, r10 = rho_np(ch, 1)
    assert r01[0].tolist() == [0, 1] and r10[0].tolist() == [0, -2]
    lanes = rho_lanes(ch, 1, 16)
    assert lanes[0, 1, :2].tolist() == [0, 1] and lanes[1, 0, :2].tolist() == [0, -2]
    # where it shows in an LLR: small estimates, a large shift, QPSK; a receiver that took conj(rho01) for layer 1 differs
    rng = np.random.default_rng(9)
    rx, ch = rand_case(rng, 2, 400, 3000)
    s = 4
    got, want = host_ml(m, rx, ch, 2, s), ml_np(rx, ch, 2, s)
    assert np.array_equal(got, want)
    r01, r10 = rho_np(ch, s)
    differs = (r10[:, 0] != r01[:, 0]) | (r10[:, 1] != R._wrap16(-r01[:, 1]))
    assert differs.sum() > 100
    from rx_front_np import compensate_np
    y = [compensate_np(rx, ch[l], 2, s)[0].astype(np.int64) for l in range(2)]
    L = R.qpsk_qpsk_lanes(y[1][:, 0], y[1][:, 1], y[0][:, 0], y[0][:, 1], r01[:, 0], R._wrap16(-r01[:, 1]))
    assert not np.array_equal(np.stack([v >> 4 for v in L], 1), want[:, 1])


def test_level_ml_host_equals_the_transcription(built):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    rng = np.random.default_rng(3)
    seen = set()
    for nb_re in (16, 48, 1, 6 * 51, 100):
        for n_rx in (1, 2, 3, 4, 8):
            for max_ch in (0, 2047, 2048, 16384, 32767):
                for amp in (32768, 1200):
                    ch = rand_case(rng, n_rx, nb_re, amp)[1]
                    stride = nb_re + int(rng.integers(0, 5))
                    a = np.zeros((2 * n_rx, stride, 2), np.int16)
                    a[:, :nb_re] = ch.reshape(2 * n_rx, nb_re, 2)
                    lv, avg = m.ulsch_level_ml_host(a, n_rx, stride, nb_re, max_ch)
                    want = level_ml_np(ch, max_ch)
                    assert lv == want[0] and np.array_equal(avg, want[1]), (nb_re, n_rx, max_ch, amp)
                    lanes = level_mmse_lanes(ch, max_ch)                    # the same averages; its formula has the MMSE's - 3
                    assert np.array_equal(avg, lanes[1]) and lv == max(0, R.log2_approx(max([0] + avg.tolist())) >> 1)
                    seen.add(lv)
    assert len(seen) > 3
    # by hand: 16 REs of (1000, 0) on every pair.  max_ch 1000: shift_ch_ext 0, h' = 1000, avg 1e6, log2_approx 20 -> 10;
    # max_ch 16384: shift_ch_ext = 4, ch_amp = 4096, b = 0: h' = 62, 16 terms of 3844 >> 4 = 240, avg 3840, log2_approx 12 -> 6
    ch = np.zeros((4, 16, 2), np.int16)
    ch[:, :, 0] = 1000
    for max_ch, lv_want, avg_want in ((1000, 10, 1000000), (16384, 6, 3840)):
        lv, avg = m.ulsch_level_ml_host(ch, 2, 16, 16, max_ch)
        assert (lv, avg.tolist()) == (lv_want, [avg_want] * 4)
    assert m.ulsch_level_ml_host(np.zeros((8, 5, 2), np.int16), 4, 5, 5, 0)[0] == 0


def test_host_checks_refuse_bad_arguments_and_the_interface_is_declared(built):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    z = np.zeros((18, 4, 2), np.int16)
    for bad, why in ((lambda: m.ulsch_ml_2layers_host(z, z, 0, 4, 4, 2, 0), "n_rx"), (lambda: m.ulsch_ml_2layers_host(z, z, 9, 4, 4, 2, 0), "n_rx"),
                     (lambda: m.ulsch_ml_2layers_host(z, z, 2, 4, 4, 6, 0), "Qm"), (lambda: m.ulsch_ml_2layers_host(z, z, 2, 4, 4, 8, 0), "Qm"),
                     (lambda: m.ulsch_ml_2layers_host(z, z, 2, 4, 4, 3, 0), "Qm"), (lambda: m.ulsch_level_ml_host(z, 0, 4, 4, 0), "n_rx"),
                     (lambda: m.ulsch_level_ml_host(z, 9, 4, 4, 0), "n_rx"), (lambda: m.ulsch_level_ml_host(z, 2, 4, 0, 0), "nb_re")):
        with pytest.raises(RuntimeError):
            bad()
        assert why in m.last_error()
    names = {"nrLDPC_hip_ulsch_channel_level_grid_ml", "nrLDPC_hip_ulsch_ml_2layers_grid", "nrLDPC_hip_ulsch_ml_2layers_host",
             "nrLDPC_hip_ulsch_level_ml_host"}
    assert set(m.EXPORTS) >= names
    header = (ROOT / "include" / "nrLDPC_hip.h").read_text()
    L = pkg.load_library()
    for n in names:
        assert n + "(" in header and getattr(L, n)


def test_header_under_the_host_sanitizers(tmp_path):
    """tests/rx_ml_check.c over the plain-C header, with -fsanitize=address,undefined: no signed overflow, no bad shift, no index
    outside rho_rs / y0_s / bit_mets"""
    exe = tmp_path / "rx_ml_check"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    str(ROOT / "openairinterface5g_amd" / "csrc"), "-o", str(exe), str(ROOT / "tests" / "rx_ml_check.c")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().isdigit(), r.stdout + r.stderr


# ---- end to end on the CPU ------------------------------------------------------------------------------------------------
# The channel is the MMSE end-to-end tests' (test_rx_mmse_host.py: every path a gain of 400..480 with a random phase, the two
# layers' columns nearly orthogonal, sigma = 3 per component): |h|^2 lies in [2^17, 2^18), so log2_approx(avgs) = 18 and, without
# the MMSE's - 3, log2_maxh = 9.  Then a layer's matched filter is about n_rx 2e5 >> 9 = 400 n_rx times the point (|point| <=
# 1.34 for 16QAM: below 2200 for n_rx = 4), mag_a about 250 n_rx, rho a few hundred: nothing near the int16 range, and the QPSK
# LLRs (>> 4) reach 40..100, the 16QAM ones several hundred.  A channel 64 times louder would saturate the matched filter, one
# 8 times fainter leaves QPSK LLRs of 2 or 3.
def ml_e2e_case(Qm, n_rx):
    """mmse_e2e_case at Qm 2 / 4: (tb, scrambling, payload, per-symbol nb_re, H, max_ch, seed for the noise)"""
    return mmse_e2e_case(Qm, n_rx)


def ml_e2e_llr(tb, syms, rx, ch, lv, receiver=ml_np):
    """the block's LLRs in codeword order (flat int16, G entries) out of the numpy receiver, symbol by symbol"""
    llr, off = np.zeros(tb["G"], np.int16), 0
    for nb in syms:
        llr_np(llr, receiver(rx[:, off:off + nb], ch[:, :, off:off + nb], tb["Qm"], lv), tb["Qm"], off)
        off += nb
    return llr


@pytest.mark.parametrize("Qm,n_rx", [(2, 2), (2, 4), (4, 2), (4, 4)])
def test_cpu_end_to_end_reference_arithmetic_decodes(built, Qm, n_rx):
    tb, scr, pay, syms, H, max_ch, seed = ml_e2e_case(Qm, n_rx)
    assert max_ch < 2048
    bits = O.dlsch_encode(tb, pay)
    planes = symbols_np(bits, scr, Qm, 2)
    rx, ch = mmse_e2e_channel(planes, H, seed)
    lv = level_ml_np(ch[:, :, :syms[0]], max_ch)[0]
    assert lv == 9
    llr = ml_e2e_llr(tb, syms, rx, ch, lv)
    assert 20 < np.abs(llr).max() < 8000
    llr = unscramble(llr, c_init_of(*scr), 0)
    s = O.segmentation(None, O.len_with_crc(1, tb["A"]), tb["BG"])
    harq = [np.zeros(66 * 384 + 16, np.int16) for _ in range(s["C"])]
    got, ack, iters, _ = O.ulsch_decode(tb, llr, harq, 8)
    assert ack and np.array_equal(got, pay), (Qm, n_rx, iters)
