"""numpy restatement of the two-layer PUSCH MMSE receiver for 64QAM / 256QAM, written from the reference's lines (openair1/PHY/
NR_TRANSPORT/nr_ulsch_demodulation.c:382-415 nr_ulsch_scale_channel, :434-466 nr_ulsch_channel_level, :505-548 the matched filter,
:580-640 nr_ulsch_det_HhH, :646-687 nr_ulsch_conjch0_mult_ch1, :689-750 nr_ulsch_comp_muli_sum, :756-867
nr_ulsch_construct_HhH_elements, :869-1260 nr_ulsch_mmse_2layers, :1431-1438 layer de-mapping, :1612-1647 the level) -- not from
csrc/nr_rx_mmse.h.  It exists twice:
  * per RE / per quad (mmse_np, level_mmse_np): the formulas in plain integer arithmetic, vectorised over the REs;
  * lane by lane (mmse_lanes, level_mmse_lanes): the 128-bit instruction sequences on the reference's zero-initialised buffers of
    buffer_length entries and its run over 12 ceil(nb_re / 12) of them.
rx = int16 [n_rx, nb_re, 2]; ch = int16 [2, n_rx, nb_re, 2] (layer, antenna: the reference's pair l n_rx + a); results int16
[2, Qm/2, nb_re, 2] = per layer y, mag_a, mag_b, mag_c.  Where the reference aborts (AssertFatal :1181) both go on with what the
instructions give."""
import numpy as np

from rx_front_np import (AMPS, _cdiv, _sat16, _wrap16, _wrap32, compensate_lanes, factor2, log2_approx, madd_epi16, packs_epi32, sign_epi16,
                         srai_epi32, unpackhi_epi32, unpacklo_epi32)


def _u32(x):
    return np.asarray(x, np.int64) & 0xffffffff


# ---------------------------------------------------------------------------------------------------------
# per RE / per quad
# ---------------------------------------------------------------------------------------------------------
def _conj_mult(h0, h1, s):
    """pack(conj(h0) h1 >> s), [n, 2] int64 (:664-674; the matched filter's term :520-530 is the same)"""
    pr = _wrap32(h0[:, 0] * h1[:, 0] + h0[:, 1] * h1[:, 1])
    pi = _wrap32(_wrap16(-h0[:, 1]) * h1[:, 0] + h0[:, 0] * h1[:, 1])
    return np.stack([_sat16(pr >> s), _sat16(pi >> s)], 1)


def _mul_re(x, y):
    return _wrap32(x[:, 0] * y[:, 0] + _wrap16(-x[:, 1]) * y[:, 1])


def _mul_im(x, y):
    return _wrap32(x[:, 1] * y[:, 0] + x[:, 0] * y[:, 1])


def _add32_packed(x, nvar):
    """add_epi32 of nvar on c16 values seen as 32-bit words (:1108-1109)"""
    w = ((x[:, 0] & 0xffff) | ((x[:, 1] & 0xffff) << 16)) + nvar & 0xffffffff
    return np.stack([_wrap16(w & 0xffff), _wrap16(w >> 16)], 1)


def _sh(x, b):
    return x >> b if b > 0 else _wrap32(x << -b)


def mmse_np(rx, ch, Qm, s, nvar):
    rx, ch = np.asarray(rx, np.int16).astype(np.int64), np.asarray(ch, np.int16).astype(np.int64)
    n_rx, nb_re = rx.shape[0], rx.shape[1]
    assert n_rx in (2, 4) and ch.shape[:2] == (2, n_rx)
    n = (nb_re + 3) & ~3                                   # whole quads; the lanes behind nb_re are zeros
    rx = np.concatenate([rx, np.zeros((n_rx, n - nb_re, 2), np.int64)], 1)
    ch = np.concatenate([ch, np.zeros((2, n_rx, n - nb_re, 2), np.int64)], 2)
    y = np.zeros((2, n, 2), np.int64)
    for l in range(2):
        for a in range(n_rx):
            y[l] = _wrap16(y[l] + _conj_mult(ch[l, a], rx[a], s))          # add_epi16 (:542)
    hhh = {}
    for name, (l0, l1) in dict(a=(0, 0), b=(0, 1), c=(1, 0), d=(1, 1)).items():
        acc = _conj_mult(ch[l0, 0], ch[l1, 0], s)
        for a in range(1, n_rx):
            acc = _sat16(acc + _conj_mult(ch[l0, a], ch[l1, a], s))         # adds_epi16, in the antennas' order (:814-828)
        hhh[name] = acc
    if nvar != 0:
        hhh["a"], hhh["d"] = _add32_packed(hhh["a"], nvar), _add32_packed(hhh["d"], nvar)
    A, B, Cc, D = hhh["a"], hhh["b"], hhh["c"], hhh["d"]
    det = _wrap32(_mul_re(A, D) - _mul_re(B, Cc))
    det = np.where(det < 0, _wrap32(-det), det)                             # abs_epi32: INT32_MIN stays
    out = np.zeros((2, Qm // 2, n, 2), np.int64)
    amps = AMPS[Qm]
    for q in range(n // 4):
        w = slice(4 * q, 4 * q + 4)
        b_mag = log2_approx(int((_u32(det[w]) >> 2).sum()) & 0xffffffff) - 8          # :1179-1185
        b_sym = log2_approx(int((det[w] >> 2).sum()) & 0xffffffff) - 8                # :726-732
        m = _sat16(_sh(det[w], b_mag))
        for k in range(1, Qm // 2):
            v = _wrap16(((m * amps[k - 1]) >> 16) << 1)                               # mulhi_epi16, slli_epi16
            out[:, k, w, 0] = out[:, k, w, 1] = v
        for l, (x, yy, ww, z) in enumerate(((y[0][w], D[w], y[1][w], B[w]), (y[1][w], A[w], y[0][w], Cc[w]))):
            re = _wrap32(_mul_re(x, yy) - _mul_re(ww, z))
            im = _wrap32(_mul_im(x, yy) - _mul_im(ww, z))
            out[l, 0, w, 0], out[l, 0, w, 1] = _sat16(_sh(re, b_sym)), _sat16(_sh(im, b_sym))
    return out[:, :, :nb_re].astype(np.int16)


def _scale_params(max_ch):
    shift_ch_ext = log2_approx((max_ch >> 11) & 0xffffffff) & 0xff           # :1614, a uint8
    b, ch_amp = 3, 1024 * 8
    if shift_ch_ext > 3:
        b = 0
        ch_amp >>= shift_ch_ext - 3
        if ch_amp == 0:
            ch_amp = 1
    else:
        b -= shift_ch_ext
    return b, ch_amp


def level_mmse_np(ch, max_ch):
    """(log2_maxh, averages) of one block's measurement symbol; ch = int16 [2, n_rx, nb_re, 2]"""
    ch = np.asarray(ch, np.int16).astype(np.int64)
    nb_re = ch.shape[2]
    ln = (nb_re + 15) & ~15
    x = factor2(ln)
    yy = ln >> x
    b, ch_amp = _scale_params(max_ch)
    avg = []
    for l in range(2):
        for a in range(ch.shape[1]):
            h = _wrap16(((ch[l, a] * ch_amp) >> 16) << b)
            t = _wrap32(h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1]) >> x
            avg.append(_cdiv(int(_wrap32(int(t.sum()))), yy))
    avgs = max([0] + avg)
    return max(0, (log2_approx(avgs) >> 1) - 3), np.array(avg, np.int32)


# ---------------------------------------------------------------------------------------------------------
# lane by lane: 128-bit vectors of 8 int16 / 4 int32 lanes
# ---------------------------------------------------------------------------------------------------------
def adds_epi16(a, b):
    return _sat16(a + b)


def mulhi_epi16(a, b):
    return (a * b) >> 16


def slli_epi16(a, n):
    return _wrap16(a << n)


def slli_epi32(a, n):
    return _wrap32(a << n)


def sub_epi32(a, b):
    return _wrap32(a - b)


def abs_epi32(a):
    return np.where(a < 0, _wrap32(-a), a)


def add_epi32_on16(a16, b32):
    """add_epi32 where the first operand is held as 8 int16 lanes"""
    w = (a16[0::2] & 0xffff) | ((a16[1::2] & 0xffff) << 16)
    w = (w + (b32 & 0xffffffff)) & 0xffffffff
    out = np.empty_like(a16)
    out[0::2], out[1::2] = _wrap16(w & 0xffff), _wrap16(w >> 16)
    return out


def shufflelo_epi16_2301(a):
    """SIMDE_MM_SHUFFLE(2,3,0,1) on the low four lanes: out = in[1], in[0], in[3], in[2]"""
    out = a.copy()
    out[0:4] = a[[1, 0, 3, 2]]
    return out


def shufflehi_epi16_2301(a):
    out = a.copy()
    out[4:8] = a[[5, 4, 7, 6]]
    return out


NR_CONJUGATE = np.array([-1, 1, -1, 1, -1, 1, -1, 1], np.int64)   # :653
NR_CONJUG2 = np.array([1, -1, 1, -1, 1, -1, 1, -1], np.int64)     # :589, :695


def conjch0_mult_ch1(ch0, ch1, nb_rb, shift):
    """:646-687 on flat int16 lanes; 3 nb_rb vectors"""
    out = np.zeros(12 * nb_rb * 2, np.int64)
    for rb in range(3 * nb_rb):
        w = slice(8 * rb, 8 * rb + 8)
        d0 = madd_epi16(ch0[w], ch1[w])
        d1 = shufflelo_epi16_2301(ch0[w])
        d1 = shufflehi_epi16_2301(d1)
        d1 = sign_epi16(d1, NR_CONJUGATE)
        d1 = madd_epi16(d1, ch1[w])
        d0 = srai_epi32(d0, shift)
        d1 = srai_epi32(d1, shift)
        d2 = unpacklo_epi32(d0, d1)
        d3 = unpackhi_epi32(d0, d1)
        out[w] = packs_epi32(d2, d3)
    return out


def comp_muli_sum(x, y, w, z, det):
    """:689-750 on one vector"""
    xy_re = madd_epi16(sign_epi16(x, NR_CONJUG2), y)
    xy_im = madd_epi16(shufflehi_epi16_2301(shufflelo_epi16_2301(x)), y)
    wz_re = madd_epi16(sign_epi16(w, NR_CONJUG2), z)
    wz_im = madd_epi16(shufflehi_epi16_2301(shufflelo_epi16_2301(w)), z)
    xy_re = sub_epi32(xy_re, wz_re)
    xy_im = sub_epi32(xy_im, wz_im)
    sum_det = 0
    for k in range(4):
        sum_det = int(_wrap32(sum_det + (int(det[k]) >> 2)))
    b = log2_approx(sum_det & 0xffffffff) - 8
    if b > 0:
        xy_re, xy_im = srai_epi32(xy_re, b), srai_epi32(xy_im, b)
    else:
        xy_re, xy_im = slli_epi32(xy_re, -b), slli_epi32(xy_im, -b)
    return packs_epi32(unpacklo_epi32(xy_re, xy_im), unpackhi_epi32(xy_re, xy_im))


def mmse_lanes(rx, ch, Qm, s, nvar):
    rx, ch = np.asarray(rx, np.int16), np.asarray(ch, np.int16)
    n_rx, nb_re = rx.shape[0], rx.shape[1]
    nb_rb_0 = nb_re // 12 + (1 if nb_re % 12 else 0)                      # :887
    bl = (12 * nb_rb_0 + 15) & ~15                                        # :1280 with rb_size = the RBs the symbol's REs fill
    n_run = 12 * nb_rb_0
    chFext = np.zeros((2, n_rx, bl, 2), np.int64)                         # :1285
    chFext[:, :, :nb_re] = ch
    # the matched filter of each layer into zeroed rxdataF_comp (:505-548, :1311): the single-layer restatement, per layer
    comp = np.zeros((2, 2 * bl), np.int64)
    for l in range(2):
        comp[l, :2 * nb_re] = compensate_lanes(rx, ch[l], 2, s, buffer_length=bl)[0].reshape(-1)
    flat = lambda l, a: chFext[l, a].reshape(-1)                          # chAL of the reference: antenna A, layer L (:917-935)
    cm = lambda p, q: conjch0_mult_ch1(flat(*p), flat(*q), nb_rb_0, s)
    ants = range(n_rx)
    c_00 = [cm((0, a), (0, a)) for a in ants]                             # conjchA0_chA0
    c_11 = [cm((1, a), (1, a)) for a in ants]                             # conjchA1_chA1
    c_01 = [cm((0, a), (1, a)) for a in ants]                             # conjchA0_chA1
    c_10 = [cm((1, a), (0, a)) for a in ants]                             # conjchA1_chA0
    af = {}
    for name, terms in (("00", c_00), ("11", c_11), ("01", c_01), ("10", c_10)):   # :812-828
        acc = np.zeros(2 * n_run, np.int64)
        for rb in range(3 * nb_rb_0):
            w = slice(8 * rb, 8 * rb + 8)
            acc[w] = adds_epi16(terms[0][w], terms[1][w])
            for t in terms[2:]:
                acc[w] = adds_epi16(acc[w], t[w])
        af[name] = acc
    if nvar != 0:                                                         # :1103-1113
        nvar_128i = np.full(4, nvar, np.int64)
        for k in range(3 * nb_rb_0):
            w = slice(8 * k, 8 * k + 8)
            af["00"][w] = add_epi32_on16(af["00"][w], nvar_128i)
            af["11"][w] = add_epi32_on16(af["11"][w], nvar_128i)
    determ_fin = np.zeros(n_run, np.int64)                                # :601-623
    for rb in range(3 * nb_rb_0):
        w, w4 = slice(8 * rb, 8 * rb + 8), slice(4 * rb, 4 * rb + 4)
        ad_re = madd_epi16(sign_epi16(af["00"][w], NR_CONJUG2), af["11"][w])
        bc_re = madd_epi16(sign_epi16(af["01"][w], NR_CONJUG2), af["10"][w])
        determ_fin[w4] = abs_epi32(sub_epi32(ad_re, bc_re))
    amps = [np.full(8, v, np.int64) for v in AMPS[Qm]]
    mag = np.zeros((2, 3, 2 * bl), np.int64)
    for rb in range(3 * nb_rb_0):                                         # :1174-1256
        w, w4 = slice(8 * rb, 8 * rb + 8), slice(4 * rb, 4 * rb + 4)
        sum_det = 0
        for k in range(4):
            sum_det = int(_wrap32(sum_det + ((int(determ_fin[w4][k]) & 0xffffffff) >> 2)))
        b = log2_approx(sum_det & 0xffffffff) - 8
        d2 = srai_epi32(determ_fin[w4], b) if b > 0 else slli_epi32(determ_fin[w4], -b)
        d3 = unpacklo_epi32(d2, d2)
        d2 = unpackhi_epi32(d2, d2)
        d2 = packs_epi32(d3, d2)
        for l in range(2):
            for k in range(3):
                mag[l, k, w] = slli_epi16(mulhi_epi16(d2, amps[k]), 1)
        d0 = comp_muli_sum(comp[0, w], af["11"][w], comp[1, w], af["01"][w], determ_fin[w4])
        d1 = comp_muli_sum(comp[1, w], af["00"][w], comp[0, w], af["10"][w], determ_fin[w4])
        comp[0, w], comp[1, w] = d0, d1
    out = np.zeros((2, Qm // 2, nb_re, 2), np.int16)
    for l in range(2):
        out[l, 0] = comp[l].reshape(bl, 2)[:nb_re]
        for k in range(1, Qm // 2):
            out[l, k] = mag[l, k - 1].reshape(bl, 2)[:nb_re]
    return out


def level_mmse_lanes(ch, max_ch):
    """:391-412 with the general shift_ch_ext, :443-461 and :1634-1647 on 128-bit vectors, len = the padded symbol (:1597)"""
    ch = np.asarray(ch, np.int16)
    n_rx, nb_re = ch.shape[1], ch.shape[2]
    ln = (nb_re + 15) & ~15
    ext = np.zeros((2 * n_rx, ln, 2), np.int64)
    ext[:, :nb_re] = ch.reshape(2 * n_rx, nb_re, 2)
    b, ch_amp = _scale_params(max_ch)
    ch_amp128 = np.full(8, ch_amp, np.int64)
    x = factor2(ln)
    y = int(_wrap16(ln >> x))
    avg = []
    for pair in range(2 * n_rx):
        ul_ch128 = ext[pair].reshape(-1, 8)
        for i in range(ln >> 2):
            ul_ch128[i] = mulhi_epi16(ul_ch128[i], ch_amp128)
            ul_ch128[i] = slli_epi16(ul_ch128[i], b)
        avg128U = np.zeros(4, np.int64)
        for i in range(ln >> 2):
            avg128U = _wrap32(avg128U + srai_epi32(madd_epi16(ul_ch128[i], ul_ch128[i]), x))
        tot = 0
        for k in range(4):
            tot = int(_wrap32(tot + int(avg128U[k])))
        avg.append(_cdiv(tot, y))
    avgs = 0
    for v in avg:
        avgs = max(avgs, v)
    log2_maxh = (log2_approx(avgs) >> 1) - 3
    if log2_maxh < 0:
        log2_maxh = 0
    return log2_maxh, np.array(avg, np.int32)


# ---------------------------------------------------------------------------------------------------------
# layer de-mapping into a symbol record
# ---------------------------------------------------------------------------------------------------------
def records_np(rec, planes, Qm, plane, sym_off, rec_off=0):
    """:1431-1438 on symbols: per-layer RE i of layer l becomes codeword symbol 2 (sym_off + i) + l of each plane.  rec = flat
    int16, planes = int16 [2, Qm/2, nb_re, 2] (mmse_np's result); the record's plane k begins at int16 rec_off + 2 k plane."""
    nb_re = planes.shape[2]
    for k in range(Qm // 2):
        v = rec[rec_off + 2 * k * plane:rec_off + 2 * (k + 1) * plane].reshape(-1, 2)
        for l in range(2):
            v[2 * sym_off + l:2 * (sym_off + nb_re) + l:2] = planes[l, k]
    return rec
