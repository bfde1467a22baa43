"""numpy restatement of the single-layer PUSCH receive front, written from the reference's lines (openair1/PHY/NR_TRANSPORT/
nr_ulsch_demodulation.c:382-415 nr_ulsch_scale_channel, :434-466 nr_ulsch_channel_level, :468-577 nr_ulsch_channel_compensation,
:1612-1647 log2_maxh in nr_rx_pusch_tp; openair1/PHY/TOOLS/log2_approx.c) -- not from csrc/nr_rx_front.h.  It exists twice:
  * per RE (compensate_np, level_np): the formulas one RE at a time, vectorised over the REs;
  * lane by lane (compensate_lanes, level_lanes): the 256-bit / 128-bit instruction sequences with the reference's zero padding
    and its accumulation into zeroed buffers, 8 (4) REs per step.
Arrays are int16 [n_rx, nb_re, 2] (re, im); results int16 [Qm/2, nb_re, 2] = y, mag_a, mag_b, mag_c."""
import numpy as np

# impl_defs_top.h:205-222
QAM16_n1 = 20724
QAM64_n1, QAM64_n2 = 20225, 10112
QAM256_n1, QAM256_n2, QAM256_n3 = 20106, 10053, 5026
AMPS = {2: (0, 0, 0), 4: (QAM16_n1, 0, 0), 6: (QAM64_n1, QAM64_n2, 0), 8: (QAM256_n1, QAM256_n2, QAM256_n3)}


def _wrap32(x):
    return ((np.asarray(x, np.int64) + 2**31) % 2**32 - 2**31).astype(np.int64)


def _wrap16(x):
    return ((np.asarray(x, np.int64) + 2**15) % 2**16 - 2**15).astype(np.int64)


def _sat16(x):
    return np.clip(np.asarray(x, np.int64), -32768, 32767)


def log2_approx(x):
    """log2_approx.c:22-38"""
    l2 = 0
    for i in range(31):
        if x & (1 << i):
            l2 = i + 1
    return l2


def factor2(x):
    """log2_approx.c:40-56"""
    i = 0
    while i < 31:
        if x & (1 << i):
            break
        i += 1
    return i


def _cdiv(a, b):
    """C division of ints: the quotient is cut toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


# ---------------------------------------------------------------------------------------------------------
# per RE
# ---------------------------------------------------------------------------------------------------------
def compensate_np(rx, ch, Qm, s):
    rx, ch = np.asarray(rx, np.int16).astype(np.int64), np.asarray(ch, np.int16).astype(np.int64)
    n_rx, nb_re = rx.shape[0], rx.shape[1]
    A = AMPS[Qm]
    comp = np.zeros((nb_re, 2), np.int64)
    mag = np.zeros((3, nb_re), np.int64)
    for a in range(n_rx):
        hr, hi, yr, yi = ch[a, :, 0], ch[a, :, 1], rx[a, :, 0], rx[a, :, 1]
        pr = _wrap32(hr * yr + hi * yi)                      # madd_epi16
        pi = _wrap32(_wrap16(-hi) * yr + hr * yi)            # sign_epi16(x, -1): -32768 stays
        c = np.stack([_sat16(pr >> s), _sat16(pi >> s)], 1)  # srai, packs
        comp = _wrap16(comp + c)                             # add_epi16
        m = _sat16(_wrap32(hr * hr + hi * hi) >> s)
        for k in range(3):
            mag[k] = _wrap16(mag[k] + _wrap16((m * A[k] + 0x4000) >> 15))  # mulhrs, add_epi16
    out = np.zeros((Qm // 2, nb_re, 2), np.int16)
    out[0] = comp
    for k in range(1, Qm // 2):
        out[k, :, 0] = out[k, :, 1] = mag[k - 1]
    return out


def level_np(ch, n_rx=None):
    """(log2_maxh, averages) of one block's measurement symbol, ch = int16 [n_rx, nb_re, 2]"""
    ch = np.asarray(ch, np.int16).astype(np.int64)
    n_rx = ch.shape[0] if n_rx is None else n_rx
    nb_re = ch.shape[1]
    ln = (nb_re + 15) & ~15
    x = factor2(ln)
    yy = ln >> x
    avg = []
    for a in range(n_rx):
        h = _wrap16(((ch[a] * 8192) >> 16) << 3)             # mulhi_epi16(h, 8192) << 3
        t = _wrap32(h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1]) >> x
        avg.append(_cdiv(int(_wrap32(int(t.sum()))), yy))
    avgs = max([0] + avg)
    return max(0, (log2_approx(avgs) >> 1) + 1 + log2_approx(n_rx >> 2)), np.array(avg, np.int32)


# ---------------------------------------------------------------------------------------------------------
# lane by lane: the instructions on vectors of int16 / int32 lanes (n 128-bit lanes of 8 int16 / 4 int32)
# ---------------------------------------------------------------------------------------------------------
def madd_epi16(a, b):
    p = a.astype(np.int64) * b.astype(np.int64)
    return _wrap32(p[0::2] + p[1::2])


def shuffle_epi8(a16, mask):
    """bytes: within each 128-bit lane, out[i] = in[mask[i] & 15] (no mask byte has bit 7 set here)"""
    b = np.asarray(a16, np.int64).astype(np.int16).view(np.uint8)
    out = np.empty_like(b)
    for lane in range(b.size // 16):
        for i in range(16):
            out[16 * lane + i] = b[16 * lane + (mask[16 * lane + i] & 15)]
    return out.view(np.int16).astype(np.int64)


def sign_epi16(a, b):
    return np.where(b < 0, _wrap16(-a), np.where(b == 0, 0, a))


def srai_epi32(a, s):
    return a >> s


def _lanes(a, n):
    return a.reshape(-1, n)


def unpacklo_epi32(a, b):
    a, b = _lanes(a, 4), _lanes(b, 4)
    return np.stack([a[:, 0], b[:, 0], a[:, 1], b[:, 1]], 1).reshape(-1)


def unpackhi_epi32(a, b):
    a, b = _lanes(a, 4), _lanes(b, 4)
    return np.stack([a[:, 2], b[:, 2], a[:, 3], b[:, 3]], 1).reshape(-1)


def packs_epi32(a, b):
    return np.concatenate([_sat16(_lanes(a, 4)), _sat16(_lanes(b, 4))], 1).reshape(-1)


def unpacklo_epi16(a, b):
    a, b = _lanes(a, 8), _lanes(b, 8)
    return np.stack([a[:, 0], b[:, 0], a[:, 1], b[:, 1], a[:, 2], b[:, 2], a[:, 3], b[:, 3]], 1).reshape(-1)


def mulhrs_epi16(a, b):
    return _wrap16((a * b + 0x4000) >> 15)


def add_epi16(a, b):
    return _wrap16(a + b)


# simde_mm256_set_epi8 / set_epi16 list the highest element first (:506-507)
COMPLEX_SHUFFLE256 = [29, 28, 31, 30, 25, 24, 27, 26, 21, 20, 23, 22, 17, 16, 19, 18, 13, 12, 15, 14, 9, 8, 11, 10, 5, 4, 7, 6, 1, 0, 3, 2][::-1]
CONJ256 = np.array([1, -1, 1, -1, 1, -1, 1, -1, 1, -1, 1, -1, 1, -1, 1, -1][::-1], np.int64)


def compensate_lanes(rx, ch, Qm, s, buffer_length=None):
    """:468-550 with rho == NULL, nrOfLayers == 1; buffer_length = (nb_re + 15) & ~15 as inner_rx sizes it (:1280), inputs zero
    padded (:1284-1285), outputs zeroed (:1307-1311)"""
    rx, ch = np.asarray(rx, np.int16), np.asarray(ch, np.int16)
    n_rx, nb_re = rx.shape[0], rx.shape[1]
    bl = (nb_re + 15) & ~15 if buffer_length is None else buffer_length
    rxFext = np.zeros((n_rx, bl, 2), np.int64)
    chFext = np.zeros((n_rx, bl, 2), np.int64)
    rxFext[:, :nb_re] = rx
    chFext[:, :nb_re] = ch
    A = AMPS[Qm]
    ampa, ampb, ampc = (np.full(16, v, np.int64) for v in A)
    rxComp = np.zeros(2 * bl, np.int64)
    maga, magb, magc = np.zeros(2 * bl, np.int64), np.zeros(2 * bl, np.int64), np.zeros(2 * bl, np.int64)
    for aarx in range(n_rx):
        rxF, chF = rxFext[aarx].reshape(-1), chFext[aarx].reshape(-1)
        for i in range(bl >> 3):
            w = slice(16 * i, 16 * i + 16)
            xmmp0 = madd_epi16(chF[w], rxF[w])
            xmmp1 = shuffle_epi8(chF[w], COMPLEX_SHUFFLE256)
            xmmp1 = sign_epi16(xmmp1, CONJ256)
            xmmp1 = madd_epi16(xmmp1, rxF[w])
            xmmp0 = srai_epi32(xmmp0, s)
            xmmp1 = srai_epi32(xmmp1, s)
            xmmp2 = unpacklo_epi32(xmmp0, xmmp1)
            xmmp3 = unpackhi_epi32(xmmp0, xmmp1)
            xmmp4 = packs_epi32(xmmp2, xmmp3)
            xmmp0 = madd_epi16(chF[w], chF[w])
            xmmp0 = srai_epi32(xmmp0, s)
            xmmp0 = packs_epi32(xmmp0, xmmp0)
            xmmp1 = unpacklo_epi16(xmmp0, xmmp0)
            xmmp2 = mulhrs_epi16(xmmp1, ampa)
            xmmp3 = mulhrs_epi16(xmmp1, ampb)
            xmmp1 = mulhrs_epi16(xmmp1, ampc)
            rxComp[w] = add_epi16(rxComp[w], xmmp4)
            if Qm > 2:
                maga[w] = add_epi16(maga[w], xmmp2)
            if Qm > 4:
                magb[w] = add_epi16(magb[w], xmmp3)
            if Qm > 6:
                magc[w] = add_epi16(magc[w], xmmp1)
    planes = [rxComp, maga, magb, magc][:Qm // 2]
    return np.stack([p.reshape(bl, 2)[:nb_re] for p in planes]).astype(np.int16)


def level_lanes(ch, n_rx=None):
    """A literal transcription of :391-412 (shift_ch_ext = 0), :443-461 and :1634-1647 on 128-bit vectors, len = the padded
    symbol (:1597), y an int16 as the reference declares it"""
    ch = np.asarray(ch, np.int16)
    n_rx = ch.shape[0] if n_rx is None else n_rx
    nb_re = ch.shape[1]
    ln = (nb_re + 15) & ~15
    ext = np.zeros((n_rx, ln, 2), np.int64)
    ext[:, :nb_re] = ch
    b, ch_amp = 3, 1024 * 8
    ch_amp128 = np.full(8, ch_amp, np.int64)
    x = factor2(ln)
    y = int(_wrap16(ln >> x))
    avg = []
    for aarx in range(n_rx):
        ul_ch128 = ext[aarx].reshape(-1, 8)
        for i in range(ln >> 2):
            ul_ch128[i] = (ul_ch128[i] * ch_amp128) >> 16        # mulhi_epi16
            ul_ch128[i] = _wrap16(ul_ch128[i] << b)              # slli_epi16
        avg128U = np.zeros(4, np.int64)
        for i in range(ln >> 2):
            avg128U = _wrap32(avg128U + srai_epi32(madd_epi16(ul_ch128[i], ul_ch128[i]), x))
        tot = int(_wrap32(int(_wrap32(int(_wrap32(int(avg128U[0]) + int(avg128U[1]))) + int(avg128U[2]))) + int(avg128U[3])))
        avg.append(_cdiv(tot, y))
    avgs = 0
    for v in avg:
        avgs = max(avgs, v)
    log2_maxh = (log2_approx(avgs) >> 1) + 1 + log2_approx(n_rx >> 2)
    if log2_maxh < 0:
        log2_maxh = 0
    return log2_maxh, np.array(avg, np.int32)
