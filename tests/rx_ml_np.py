"""numpy restatement of the two-layer PUSCH max-log ML receiver for QPSK / 16QAM, written from the reference's lines (openair1/PHY/
NR_TRANSPORT/nr_ulsch_demodulation.c:505-571 the compensation with rho, :1431-1438 layer de-mapping, :1612-1647 the level;
nr_ulsch_llr_computation.c:528-682 nr_ulsch_qpsk_qpsk, :820-884 the helpers, :1124-1350 nr_ulsch_qam16_qam16, :2076-2098
nr_ulsch_shift_llr, :2100-2129 nr_ulsch_compute_ML_llr; openair1/PHY/TOOLS/simde_operations.c:40-60) -- not from csrc/nr_rx_ml.h.
It exists twice:
  * per RE (ml_np, level_ml_np): the formulas in plain integer arithmetic, vectorised over the REs, every RE computed once;
  * lane by lane (ml_lanes): the 256-bit instruction sequences over zero-initialised buffers of buffer_length entries, with the
    reference's loop bounds (`for (i = 0; i < length >> 3; i += 2)`), its stores and nr_ulsch_shift_llr's ranges.
rx = int16 [n_rx, nb_re, 2]; ch = int16 [2, n_rx, nb_re, 2] (layer, antenna: the reference's pair l n_rx + a).  ml_np returns int16
[nb_re, 2, Qm]: per RE and layer the Qm LLRs, which flattened is the codeword's order (:1431-1438)."""
import numpy as np

from rx_front_np import (AMPS, COMPLEX_SHUFFLE256, CONJ256, _sat16, _wrap16, _wrap32, compensate_lanes, compensate_np, log2_approx, madd_epi16,
                         packs_epi32, shuffle_epi8, sign_epi16, srai_epi32, unpackhi_epi32, unpacklo_epi32)
from rx_mmse_np import _conj_mult, level_mmse_np


# ---------------------------------------------------------------------------------------------------------
# int16 instructions; they work on arrays of any shape, one lane per element
# ---------------------------------------------------------------------------------------------------------
SATURATED = {"adds": 0, "subs": 0}    # lanes in which adds / subs clamped, counted since the caller last reset them


def _count(kind, v):
    SATURATED[kind] += int(np.count_nonzero((np.asarray(v) > 32767) | (np.asarray(v) < -32768)))
    return _sat16(v)


def adds(a, b):
    return _count("adds", a + b)


def subs(a, b):
    return _count("subs", a - b)


def abs16(a):
    return np.where(a < 0, _wrap16(-a), a)          # abs_epi16(-32768) = -32768


def mulhi(a, b):
    return (a * b) >> 16


def slli(a, n):
    return _wrap16(a << n)


def srai(a, n):
    return a >> n


# ---------------------------------------------------------------------------------------------------------
# the two LLR functions on separated lanes: shared by both restatements (a lane is an RE in both)
# ---------------------------------------------------------------------------------------------------------
def qpsk_qpsk_lanes(y0r, y0i, y1r, y1i, rhor, rhoi):
    """:540-666; returns (L1, L2) before nr_ulsch_shift_llr"""
    K = 23170
    y0r_over2 = slli(mulhi(y0r, K), 1)
    y0i_over2 = slli(mulhi(y0i, K), 1)
    y1r_over2 = srai(y1r, 1)
    y1i_over2 = srai(y1i, 1)
    rho_p = mulhi(adds(rhor, rhoi), K)
    rho_m = mulhi(subs(rhor, rhoi), K)
    abs_psi_rpm = abs16(subs(rho_p, y1r_over2))
    abs_psi_imm = abs16(subs(rho_m, y1i_over2))
    abs_psi_rmm = abs16(subs(rho_m, y1r_over2))
    abs_psi_ipm = abs16(subs(rho_p, y1i_over2))
    abs_psi_rpp = abs16(adds(rho_p, y1r_over2))
    abs_psi_imp = abs16(adds(rho_m, y1i_over2))
    abs_psi_rmp = abs16(adds(rho_m, y1r_over2))
    abs_psi_ipp = abs16(adds(rho_p, y1i_over2))
    bit_met_num_re_p = adds(adds(adds(abs_psi_rpm, abs_psi_imm), y0r_over2), y0i_over2)
    bit_met_num_re_m = subs(adds(adds(abs_psi_rmm, abs_psi_ipp), y0r_over2), y0i_over2)
    bit_met_den_re_p = adds(subs(adds(abs_psi_rmp, abs_psi_ipm), y0r_over2), y0i_over2)
    bit_met_den_re_m = subs(subs(adds(abs_psi_rpp, abs_psi_imp), y0r_over2), y0i_over2)
    bit_met_num_im_p = adds(adds(adds(abs_psi_rpm, abs_psi_imm), y0r_over2), y0i_over2)
    bit_met_num_im_m = adds(subs(adds(abs_psi_rmp, abs_psi_ipm), y0r_over2), y0i_over2)
    bit_met_den_im_p = subs(adds(adds(abs_psi_rmm, abs_psi_ipp), y0r_over2), y0i_over2)
    bit_met_den_im_m = subs(subs(adds(abs_psi_rpp, abs_psi_imp), y0r_over2), y0i_over2)
    logmax_num_re0 = np.maximum(bit_met_num_re_p, bit_met_num_re_m)
    logmax_den_re0 = np.maximum(bit_met_den_re_p, bit_met_den_re_m)
    logmax_num_im0 = np.maximum(bit_met_num_im_p, bit_met_num_im_m)
    logmax_den_im0 = np.maximum(bit_met_den_im_p, bit_met_den_im_m)
    return subs(logmax_num_re0, logmax_den_re0), subs(logmax_num_im0, logmax_den_im0)


def _interference_abs(psi, int_ch_mag, c1, c2):
    return np.where(int_ch_mag > psi, c1, c2)                                   # :830-837


def _prodsum_psi_a(psi_r, a_r, psi_i, a_i):
    return adds(slli(mulhi(psi_r, a_r), 1), slli(mulhi(psi_i, a_i), 1))         # :820-827


def _square_a(a_r, a_i, int_ch_mag, scale_factor):
    t = slli(mulhi(slli(mulhi(slli(mulhi(a_r, a_r), 1), scale_factor), 1), int_ch_mag), 1)
    t2 = slli(mulhi(slli(mulhi(slli(mulhi(a_i, a_i), 1), scale_factor), 1), int_ch_mag), 1)
    return adds(t, t2)                                                          # :840-855


def _max8(*m):
    out = m[0]
    for v in m[1:]:
        out = np.maximum(out, v)
    return out


def qam16_qam16_lanes(y0r, y0i, y1r, y1i, ch_mag_des, ch_mag_int, rhor, rhoi):
    """:1174-1324; returns (L1, L2, L3, L4) = (y0r, y1r, y0i, y1i) of :1321-1324"""
    ONE_OVER_SQRT_10, ONE_OVER_SQRT_10_Q15, THREE_OVER_SQRT_10 = 20724, 10362, 31086
    SQRT_10_OVER_FOUR, ONE_OVER_TWO_SQRT_10, NINE_OVER_TWO_SQRT_10 = 25905, 10362, 23315
    rho_rpi, rho_rmi = adds(rhor, rhoi), subs(rhor, rhoi)
    rho_rs = [None] * 8
    rho_rs[0] = mulhi(rho_rpi, ONE_OVER_SQRT_10)
    rho_rs[4] = mulhi(rho_rmi, ONE_OVER_SQRT_10)
    rho_rs[3] = slli(mulhi(rho_rpi, THREE_OVER_SQRT_10), 1)
    rho_rs[7] = slli(mulhi(rho_rmi, THREE_OVER_SQRT_10), 1)
    xmm4 = mulhi(rhor, ONE_OVER_SQRT_10)
    xmm5 = slli(mulhi(rhoi, THREE_OVER_SQRT_10), 1)
    rho_rs[1], rho_rs[5] = adds(xmm4, xmm5), subs(xmm4, xmm5)
    xmm6 = slli(mulhi(rhor, THREE_OVER_SQRT_10), 1)
    xmm7 = mulhi(rhoi, ONE_OVER_SQRT_10)
    rho_rs[2], rho_rs[6] = adds(xmm6, xmm7), subs(xmm6, xmm7)
    psi_rs, psi_is = [None] * 16, [None] * 16
    for j in range(8):
        psi_rs[j] = abs16(subs(rho_rs[j], y1r))
    for j in range(8, 16):
        psi_rs[j] = abs16(adds(rho_rs[(j - 4) & 7], y1r))
    rho_rs_indexes = [4, 6, 5, 7, 0, 2, 1, 3, 0, 2, 1, 3, 4, 6, 5, 7]
    for k in range(0, 16, 8):
        for j in range(k, k + 4):
            psi_is[j] = abs16(subs(rho_rs[rho_rs_indexes[j]], y1i))
            psi_is[j + 4] = abs16(adds(rho_rs[rho_rs_indexes[j + 4]], y1i))
    y0r_over_sqrt10, y0i_over_sqrt10 = mulhi(y0r, ONE_OVER_SQRT_10), mulhi(y0i, ONE_OVER_SQRT_10)
    y0r_three_over_sqrt10 = slli(mulhi(y0r, THREE_OVER_SQRT_10), 1)
    y0i_three_over_sqrt10 = slli(mulhi(y0i, THREE_OVER_SQRT_10), 1)
    y0_s = [None] * 8
    y0_s[0], y0_s[4] = adds(y0r_over_sqrt10, y0i_over_sqrt10), subs(y0r_over_sqrt10, y0i_over_sqrt10)
    y0_s[1], y0_s[5] = adds(y0r_over_sqrt10, y0i_three_over_sqrt10), subs(y0r_over_sqrt10, y0i_three_over_sqrt10)
    y0_s[2], y0_s[6] = adds(y0r_three_over_sqrt10, y0i_over_sqrt10), subs(y0r_three_over_sqrt10, y0i_over_sqrt10)
    y0_s[3], y0_s[7] = adds(y0r_three_over_sqrt10, y0i_three_over_sqrt10), subs(y0r_three_over_sqrt10, y0i_three_over_sqrt10)
    psi_as, a_sqs = [None] * 16, [None] * 16
    for j in range(16):
        a_r = _interference_abs(psi_rs[j], ch_mag_int, ONE_OVER_SQRT_10_Q15, THREE_OVER_SQRT_10)
        a_i = _interference_abs(psi_is[j], ch_mag_int, ONE_OVER_SQRT_10_Q15, THREE_OVER_SQRT_10)
        psi_as[j] = _prodsum_psi_a(psi_rs[j], a_r, psi_is[j], a_i)
        a_sqs[j] = _square_a(a_r, a_i, ch_mag_int, SQRT_10_OVER_FOUR)
    ch_mag_over_10 = mulhi(ch_mag_des, ONE_OVER_TWO_SQRT_10)
    ch_mag_over_2 = slli(mulhi(ch_mag_des, SQRT_10_OVER_FOUR), 1)
    ch_mag_9_over_10 = slli(mulhi(ch_mag_des, NINE_OVER_TWO_SQRT_10), 2)
    tail = [ch_mag_over_10, ch_mag_over_2, ch_mag_over_2, ch_mag_9_over_10]
    b = [None] * 16
    for j in range(0, 8, 4):
        for t in range(4):
            b[j + t] = subs(adds(subs(psi_as[j + t], a_sqs[j + t]), y0_s[j + t]), tail[t])
    for j in range(8, 16, 4):
        for t in range(4):
            b[j + t] = subs(subs(subs(psi_as[j + t], a_sqs[j + t]), y0_s[(j - 4 + t) & 7]), tail[t])
    logmax_num_re0 = _max8(b[8], b[9], b[10], b[11], b[12], b[13], b[14], b[15])
    logmax_den_re0 = _max8(b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7])
    logmax_num_re1 = _max8(b[4], b[5], b[6], b[7], b[12], b[13], b[14], b[15])
    logmax_den_re1 = _max8(b[0], b[1], b[3], b[2], b[8], b[9], b[10], b[11])
    logmax_num_im0 = _max8(b[2], b[3], b[6], b[7], b[10], b[11], b[14], b[15])
    logmax_den_im0 = _max8(b[0], b[1], b[4], b[5], b[8], b[9], b[12], b[13])
    logmax_num_im1 = _max8(b[1], b[3], b[5], b[7], b[9], b[11], b[13], b[15])
    logmax_den_im1 = _max8(b[0], b[2], b[4], b[6], b[8], b[10], b[12], b[14])
    return (subs(logmax_den_re0, logmax_num_re0), subs(logmax_den_re1, logmax_num_re1), subs(logmax_den_im0, logmax_num_im0),
            subs(logmax_den_im1, logmax_num_im1))


# ---------------------------------------------------------------------------------------------------------
# per RE
# ---------------------------------------------------------------------------------------------------------
def rho_np(ch, s):
    """(rho[0][1], rho[1][0]), int64 [nb_re, 2] each: the saturating sums over the antennas, in order (:550-570)"""
    ch = np.asarray(ch, np.int16).astype(np.int64)
    out = []
    for l0, l1 in ((0, 1), (1, 0)):
        acc = np.zeros((ch.shape[2], 2), np.int64)
        for a in range(ch.shape[1]):
            acc = _sat16(acc + _conj_mult(ch[l0, a], ch[l1, a], s))
        out.append(acc)
    return out


def ml_np(rx, ch, Qm, s):
    assert Qm in (2, 4)
    rx, ch = np.asarray(rx, np.int16), np.asarray(ch, np.int16)
    nb_re = rx.shape[1]
    comp = [compensate_np(rx, ch[l], Qm, s).astype(np.int64) for l in range(2)]   # per layer: y and, for 16QAM, mag_a (:509-548)
    rho = rho_np(ch, s)
    out = np.zeros((nb_re, 2, Qm), np.int64)
    for l in range(2):
        y0, y1, r = comp[l][0], comp[l ^ 1][0], rho[l]
        if Qm == 2:
            L = qpsk_qpsk_lanes(y0[:, 0], y0[:, 1], y1[:, 0], y1[:, 1], r[:, 0], r[:, 1])
            L = [v >> 4 for v in L]                                  # nr_ulsch_shift_llr, once
        else:
            L = qam16_qam16_lanes(y0[:, 0], y0[:, 1], y1[:, 0], y1[:, 1], comp[l][1][:, 0], comp[l ^ 1][1][:, 0], r[:, 0], r[:, 1])
        for m in range(Qm):
            out[:, l, m] = L[m]
    return out.astype(np.int16)


def level_ml_np(ch, max_ch):
    """(log2_maxh, averages): the MMSE level's averages with the formula of :1639 alone"""
    _, avg = level_mmse_np(ch, max_ch)
    avgs = max([0] + [int(v) for v in avg])
    return max(0, log2_approx(avgs) >> 1), avg


def llr_np(llr, L, Qm, sym_off, rec_off=0):
    """layer de-mapping (:1431-1438): L = int16 [nb_re, 2, Qm] (ml_np's result) into the flat int16 LLR array"""
    n = L.shape[0]
    llr[rec_off + 2 * Qm * sym_off:rec_off + 2 * Qm * (sym_off + n)] = L.reshape(-1)
    return llr


# ---------------------------------------------------------------------------------------------------------
# lane by lane: 256-bit vectors of 16 int16 lanes
# ---------------------------------------------------------------------------------------------------------
def _per128(a, fn):
    return np.concatenate([fn(a[0:8]), fn(a[8:16])])


def shufflelo_epi16_d8(a):
    return _per128(a, lambda v: np.concatenate([v[[0, 2, 1, 3]], v[4:8]]))


def shufflehi_epi16_d8(a):
    return _per128(a, lambda v: np.concatenate([v[0:4], v[[4, 6, 5, 7]]]))


def shuffle_epi32_d8(a):
    return _per128(a, lambda v: v.reshape(4, 2)[[0, 2, 1, 3]].reshape(-1))


def unpacklo_epi64(a, b):
    return np.concatenate([a[0:4], b[0:4], a[8:12], b[8:12]])


def unpackhi_epi64(a, b):
    return np.concatenate([a[4:8], b[4:8], a[12:16], b[12:16]])


def permute4x64_d8(a):
    return a.reshape(4, 4)[[0, 2, 1, 3]].reshape(-1)


def separate_real_imag_parts(in0, in1):
    """simde_operations.c:40-60: two vectors of 8 c16 -> (re, im) of the 16 REs, in order"""
    in0 = shuffle_epi32_d8(shufflehi_epi16_d8(shufflelo_epi16_d8(in0)))
    in1 = shuffle_epi32_d8(shufflehi_epi16_d8(shufflelo_epi16_d8(in1)))
    return permute4x64_d8(unpacklo_epi64(in0, in1)), permute4x64_d8(unpackhi_epi64(in0, in1))


def mm_unpacklo_epi16(a, b):
    return np.stack([a[0:4], b[0:4]], 1).reshape(-1)


def mm_unpackhi_epi16(a, b):
    return np.stack([a[4:8], b[4:8]], 1).reshape(-1)


def mm_unpacklo_epi32(a, b):
    a, b = a.reshape(4, 2), b.reshape(4, 2)
    return np.concatenate([a[0], b[0], a[1], b[1]])


def mm_unpackhi_epi32(a, b):
    a, b = a.reshape(4, 2), b.reshape(4, 2)
    return np.concatenate([a[2], b[2], a[3], b[3]])


def rho_lanes(ch, s, bl):
    """:550-570 on zero-padded chFext and zeroed rho (:1285, :1306); returns rho[2][2] as flat int16 lanes of bl c16"""
    ch = np.asarray(ch, np.int16)
    n_rx, nb_re = ch.shape[1], ch.shape[2]
    chFext = np.zeros((2, n_rx, bl, 2), np.int64)
    chFext[:, :, :nb_re] = ch
    rho = np.zeros((2, 2, 2 * bl), np.int64)
    for aatx in range(2):
        for aarx in range(n_rx):
            for atx in range(2):
                chF, chF2 = chFext[aatx, aarx].reshape(-1), chFext[atx, aarx].reshape(-1)
                for i in range(bl >> 3):
                    w = slice(16 * i, 16 * i + 16)
                    xmmp0 = madd_epi16(chF[w], chF2[w])
                    xmmp1 = shuffle_epi8(chF[w], COMPLEX_SHUFFLE256)
                    xmmp1 = sign_epi16(xmmp1, CONJ256)
                    xmmp1 = madd_epi16(xmmp1, chF2[w])
                    xmmp0 = srai_epi32(xmmp0, s)
                    xmmp1 = srai_epi32(xmmp1, s)
                    xmmp2 = unpacklo_epi32(xmmp0, xmmp1)
                    xmmp3 = unpackhi_epi32(xmmp0, xmmp1)
                    rho[aatx, atx, w] = adds(rho[aatx, atx, w], packs_epi32(xmmp2, xmmp3))
    return rho


def ml_lanes(rx, ch, Qm, s, mem_offset=0):
    """inner_rx's path for two layers below 64QAM on one symbol (:1280-1361) and nr_ulsch_compute_ML_llr.  mem_offset = the c16
    between the symbol's first LLR of a layer and the next 16-byte boundary (:2081), which depends on the buffer's address.
    Returns (llr, stored, shifted): llr = int16 [2, Qm (bl + 16)] the per-layer LLR buffers from the symbol's offset on, zero where
    nothing was stored; stored / shifted = int [bl + 16] how often each RE of a layer was stored / shifted."""
    assert Qm in (2, 4)
    rx, ch = np.asarray(rx, np.int16), np.asarray(ch, np.int16)
    nb_re = rx.shape[1]
    bl = (nb_re + 15) & ~15
    comp, mag = np.zeros((2, 2 * bl), np.int64), np.zeros((2, 2 * bl), np.int64)
    for l in range(2):
        planes = compensate_lanes(rx, ch[l], Qm, s, buffer_length=bl)     # the padding's inputs are zero: so are its outputs
        comp[l, :2 * nb_re] = planes[0].reshape(-1)
        if Qm > 2:
            mag[l, :2 * nb_re] = planes[1].reshape(-1)
    rho = rho_lanes(ch, s, bl)
    n_out = bl + 16
    llr = np.zeros((2, Qm * n_out), np.int64)
    stored, shifted = np.zeros(n_out, np.int64), np.zeros(n_out, np.int64)
    for l in range(2):                                                     # :2115-2121
        s0, s1, m0, m1, r01 = comp[l], comp[l ^ 1], mag[l], mag[l ^ 1], rho[l, l ^ 1]
        v = lambda arr, i: arr[16 * i:16 * i + 16]
        for i in range(0, nb_re >> 3, 2):
            y0r, y0i = separate_real_imag_parts(v(s0, i), v(s0, i + 1))
            y1r, y1i = separate_real_imag_parts(v(s1, i), v(s1, i + 1))
            rhor, rhoi = separate_real_imag_parts(v(r01, i), v(r01, i + 1))
            if Qm == 2:
                L1, L2 = qpsk_qpsk_lanes(y0r, y0i, y1r, y1i, rhor, rhoi)
                o = llr[l, 16 * i:]                                        # stream0_256i_out[i]
                o[0:8] = mm_unpacklo_epi16(L1[0:8], L2[0:8])               # :672-673
                o[8:16] = mm_unpackhi_epi16(L1[0:8], L2[0:8])
                n_st = 8
                if i < (nb_re >> 2) - 1:                                   # :676
                    o[16:24] = mm_unpacklo_epi16(L1[8:16], L2[8:16])
                    o[24:32] = mm_unpackhi_epi16(L1[8:16], L2[8:16])
                    n_st = 16
            else:
                des, _ = separate_real_imag_parts(v(m0, i), v(m0, i + 1))
                intf, _ = separate_real_imag_parts(v(m1, i), v(m1, i + 1))
                L1, L2, L3, L4 = qam16_qam16_lanes(y0r, y0i, y1r, y1i, des, intf, rhor, rhoi)
                o = llr[l, 32 * i:]                                        # stream0_256i_out[2 i]
                for h in range(2):                                         # :1332-1349
                    q = slice(8 * h, 8 * h + 8)
                    xmm0, xmm1 = mm_unpacklo_epi16(L1[q], L2[q]), mm_unpackhi_epi16(L1[q], L2[q])
                    xmm2, xmm3 = mm_unpacklo_epi16(L3[q], L4[q]), mm_unpackhi_epi16(L3[q], L4[q])
                    oo = o[32 * h:]
                    oo[0:8] = mm_unpacklo_epi32(xmm0, xmm2)
                    oo[8:16] = mm_unpackhi_epi32(xmm0, xmm2)
                    oo[16:24] = mm_unpacklo_epi32(xmm1, xmm3)
                    oo[24:32] = mm_unpackhi_epi32(xmm1, xmm3)
                n_st = 16
            if l == 0:
                stored[8 * i:8 * i + n_st] += 1
    if Qm == 2:                                                            # :2117, :2076-2098 with shift 4
        for i in range(mem_offset):                                        # c16Shift of one c16 = one RE's two LLRs
            llr[:, 2 * i:2 * i + 2] >>= 4
            shifted[i] += 1
        for i in range(nb_re >> 2):                                        # one 128-bit vector = four REs
            a = 2 * mem_offset + 8 * i
            llr[:, a:a + 8] >>= 4
            shifted[mem_offset + 4 * i:mem_offset + 4 * i + 4] += 1
    return llr.astype(np.int16), stored, shifted
