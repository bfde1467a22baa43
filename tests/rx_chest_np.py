"""A literal Python restatement of the reference's PUSCH channel estimation, loop by loop, for the tests to compare csrc/nr_chest.h
against.  Line numbers: openair1/PHY/NR_ESTIMATION/nr_ul_channel_estimation.c unless another file is named.  It keeps the running
ul_ch pointer and the pilot_cnt branches of TYPE1_INTERP, the saturating adds in loop order, the spill behind the allocation and,
behind `literal_type2_avg`, the two TYPE2_AVG defects.  The Gold sequence is a plain bit-by-bit LFSR, independent of csrc/nr_gold.h.
Values are Python ints; a c16 is a pair (r, i)."""
import functools
import math

MAX_DELAY_COMP = 20


def s16(x):                                   # (int16_t) cast
    return ((x + 32768) & 0xffff) - 32768


def sat16(x):                                 # adds_epi16
    return max(-32768, min(32767, x))


def mulhrs(a, b):                             # simde_mm256_mulhrs_epi16
    return s16((a * b + 0x4000) >> 15)


def c32_mul_shift(a, b, s):                   # tools_defs.h:233-238
    return ((a[0] * b[0] - a[1] * b[1]) >> s, (a[0] * b[1] + a[1] * b[0]) >> s)


def c16_mul_shift(a, b, s):                   # tools_defs.h:207-212
    r = c32_mul_shift(a, b, s)
    return (s16(r[0]), s16(r[1]))


def c16_div(a, d):                            # tools_defs.h:247-252: C division truncates towards zero
    q = lambda x: s16(int(math.trunc(x / d)) if abs(x) < 2 ** 50 else 0)
    return (q(a[0]), q(a[1]))


@functools.lru_cache(maxsize=64)
def gold_bits(c_init, n):
    """c(0 .. n - 1) of 38.211 5.2.1, bit by bit, Nc = 1600"""
    x1 = [1] + [0] * 30
    x2 = [(c_init >> k) & 1 for k in range(31)]
    for k in range(1600 + n - 31):
        x1.append(x1[k + 3] ^ x1[k])
        x2.append(x2[k + 3] ^ x2[k + 2] ^ x2[k + 1] ^ x2[k])
    return tuple(x1[1600 + k] ^ x2[1600 + k] for k in range(n))


def c_init_pusch(slot, symbol, nid, nscid):   # nr_gold.c:107-108
    return ((1 << 17) * (14 * slot + symbol + 1) * ((nid << 1) + 1) + ((nid << 1) + nscid)) % (1 << 31)


# nr_dmrs_rx.c:44-57
delta1 = [0, 0, 1, 1, 0, 0, 1, 1]
wf1 = [[1, 1], [1, -1]] * 4
wf2 = [[1, 1], [1, -1]] * 6
nr_rx_mod_table = [0, 0, 23170, -23170, -23170, 23170, 23170, -23170, 23170, 23170, -23170, -23170, -23170, 23170]
NR_MOD_TABLE_QPSK_OFFSET = 3


def pusch_dmrs_rx(c_init, p, nb_pusch_rb, re_offset, dmrs_type, n_pilots=None):
    """nr_pusch_dmrs_rx (nr_dmrs_rx.c:67-116), lp = 0; dmrs_type 0 = type 1.  n_pilots overrides nb_pusch_rb * nb_dmrs."""
    wf = wf1 if dmrs_type == 0 else wf2
    dmrs_offset = re_offset // (2 if dmrs_type == 0 else 3)                                  # :84
    nb_dmrs = 6 if dmrs_type == 0 else 4
    n = nb_pusch_rb * nb_dmrs if n_pilots is None else n_pilots
    gold = gold_bits(c_init, 2 * (dmrs_offset + n) + 2)
    out = []
    for i in range(dmrs_offset, dmrs_offset + n):                                            # :92
        w = wf[p][i & 1] * 1                                                                 # :94, wt[p][0] = 1
        idx = (gold[i << 1] << 1) ^ gold[(i << 1) + 1]                                       # :97
        r, im = nr_rx_mod_table[(NR_MOD_TABLE_QPSK_OFFSET + idx) << 1], nr_rx_mod_table[((NR_MOD_TABLE_QPSK_OFFSET + idx) << 1) + 1]
        out.append((r, im) if w == 1 else (-r, -im))                                         # :95 nr_rx_nmod_table = -nr_rx_mod_table
    return out


def c_round(x):                               # C round(): halves away from zero
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def delay_row(N, delay):                      # init_delay_table, common/utils/nr/nr_common.c:916-928
    return [(s16(c_round(256 * math.cos(2.0 * math.pi * k * delay / N))), s16(c_round(256 * math.sin(2.0 * math.pi * k * delay / N)))) for k in range(N)]


def get_delay_idx(delay):                     # nr_common.c:906-914
    return min(max(MAX_DELAY_COMP + delay, 0), MAX_DELAY_COMP << 1)


def delay_table_row(N, delay):
    """delay_table[get_delay_idx(delay)]"""
    return delay_row(N, get_delay_idx(delay) - MAX_DELAY_COMP)


filt16_ul_p0 = [4096] * 8 + [0] * 8                                                           # filt16a_32.h:242-251
filt16_ul_p1p2 = [4096] * 4 + [2048] * 8 + [0] * 4
filt16_ul_middle = [2048] * 16
filt16_ul_last = [4096] * 4 + [8192] * 4 + [0] * 8
filt8_rep4 = [16384] * 4 + [0] * 4


def multadd_vect_real_complex(x, alpha, y, at, terms=None):
    """c16multaddVectRealComplex(x, alpha, y + at, 16) (tools_defs.h:266-298); terms collects (index, y before, t) of non-zero t"""
    for k in range(16):
        v = []
        for c in range(2):
            m = mulhrs(alpha[c], x[k])
            t = sat16(m + m)
            if terms is not None and t != 0:
                terms.append((at + k, c, y[at + k][c], t))
            v.append(sat16(t + y[at + k][c]))
        y[at + k] = (v[0], v[1])


def pusch_channel_estimation(rxdataF, soffset, N, k0, nb_rb, p, dmrs_type, chest_freq, c_init, re_offset, est_delay, literal_type2_avg=True, terms=None):
    """One antenna of nr_pusch_channel_estimation (:155-450): rxdataF = list of c16 pairs (the antenna's buffer, symbol_offset
    folded into soffset), k0 = bwp_start_subcarrier, re_offset = 12 (bwp_start + rb_start).  Returns ul_ch from ch_offset on, N + 32
    entries, zeroed as by :159 (the slack takes what the reference writes behind the allocation)."""
    nushift = (p >> 1) & 1                                                                   # :89
    nb_dmrs = 6 if dmrs_type == 0 else 4
    # the averaging branches run their "last PRB" code for nb_rb = 1 too and read pilots the generator did not write: zeros here
    pilot = pusch_dmrs_rx(c_init, p, nb_rb, re_offset, dmrs_type) + [(0, 0)] * nb_dmrs
    ul_ch = [(0, 0)] * (N + 32)
    ul_ls_est = [(0, 0)] * (N + 32)                                                          # :150-151 (per call; one antenna here)
    at = 0                                                                                   # the running ul_ch pointer
    if dmrs_type == 0 and chest_freq == 0:                                                   # :167
        pil = 0
        pilot_cnt = 0
        delta = delta1[p]
        for n in range(3 * nb_rb):                                                           # :176
            ch = (0, 0)
            for k_line in range(2):
                re = (k0 + (n << 2) + (k_line << 1) + delta) % N                             # :181
                t = c32_mul_shift(pilot[pil], rxdataF[soffset + re], 16)
                ch = (t[0] + ch[0], t[1] + ch[1])                                            # c32x16maddShift
                pil += 1
            ch16 = (s16(ch[0]), s16(ch[1]))                                                  # :186
            for k in range(pilot_cnt << 1, (pilot_cnt << 1) + 4):
                ul_ls_est[k] = ch16
            pilot_cnt += 2
        tab = delay_table_row(N, est_delay)                                                  # :195-196
        pilot_cnt = 0
        for n in range(3 * nb_rb):                                                           # :203
            for k_line in range(2):
                k = pilot_cnt << 1
                ch16 = c16_mul_shift(ul_ls_est[k], tab[k], 8)                                # :210
                if pilot_cnt == 0:
                    multadd_vect_real_complex(filt16_ul_p0, ch16, ul_ch, at, terms)
                elif pilot_cnt == 1 or pilot_cnt == 2:
                    multadd_vect_real_complex(filt16_ul_p1p2, ch16, ul_ch, at, terms)
                elif pilot_cnt == 6 * nb_rb - 1:
                    multadd_vect_real_complex(filt16_ul_last, ch16, ul_ch, at, terms)
                else:
                    multadd_vect_real_complex(filt16_ul_middle, ch16, ul_ch, at, terms)
                    if pilot_cnt % 2 == 0:
                        at += 4                                                              # :228
                pilot_cnt += 1
        inv = delay_table_row(N, -est_delay)                                                 # :239-240
        pilot_cnt = 0
        for n in range(3 * nb_rb):                                                           # :241
            for k_line in range(2):
                k = pilot_cnt << 1
                ul_ch[k] = c16_mul_shift(ul_ch[k], inv[k], 8)
                ul_ch[k + 1] = c16_mul_shift(ul_ch[k + 1], inv[k + 1], 8)
                pilot_cnt += 1
    elif dmrs_type == 1 and chest_freq == 0:                                                 # :259
        pil = 0
        rx = soffset + nushift                                                               # :262
        for n in range(0, nb_rb * 12, 6):
            ch0 = c16_mul_shift(pilot[pil], rxdataF[rx + (k0 + n) % N], 15)
            pil += 1
            ch1 = c16_mul_shift(pilot[pil], rxdataF[rx + (k0 + n + 1) % N], 15)
            pil += 1
            ch = (s16((ch0[0] + ch1[0]) >> 1), s16((ch0[1] + ch1[1]) >> 1))                  # c16addShift
            # multadd_real_four_symbols_vector_complex_scalar (tools_defs.h:312-329), mulhi_s1 = mulhi << 2 (tools_defs.h:47)
            yr = [s16(((ch[0] * x) >> 16) << 2) for x in filt8_rep4]
            yi = [s16(((ch[1] * x) >> 16) << 2) for x in filt8_rep4]
            for j in range(4):
                y = ul_ls_est[n + j]
                y = (sat16(y[0] + yr[j]), sat16(y[1] + yi[j]))                               # unpacklo
                ul_ls_est[n + j] = (sat16(y[0] + yr[4 + j]), sat16(y[1] + yi[4 + j]))        # unpackhi
            ul_ls_est[n + 4] = ch
            ul_ls_est[n + 5] = ch
        tab = delay_table_row(N, -est_delay)                                                 # :279-280
        for n in range(nb_rb * 12):
            ul_ch[n] = c16_mul_shift(ul_ls_est[n], tab[n % 6], 8)
    elif dmrs_type == 0:                                                                     # :287, NO_INTERP
        rxF = soffset + nushift
        state = {"pil": 0, "re": k0}

        def cumul():                                                                         # :45-65
            c = (0, 0)
            for _ in range(6):
                t = c32_mul_shift(pilot[state["pil"]] if state["pil"] < len(pilot) else (0, 0), rxdataF[rxF + state["re"]], 15)
                c = (t[0] + c[0], t[1] + c[1])
                state["pil"] += 1
                state["re"] = (state["re"] + 2) % N
            return c16_div(c, 6)
        ch = cumul()                                                                         # :295
        for _ in range(12):
            ul_ch[at] = ch
            at += 1
        for pilot_cnt in range(6, 6 * (nb_rb - 1), 6):                                       # :309
            ch = cumul()
            for _ in range(12):
                ul_ch[at] = ch
                at += 1
        ch = cumul()                                                                         # :330, also when nb_rb = 1
        for _ in range(12):
            ul_ch[at] = ch
            at += 1
    else:                                                                                    # :344
        so = 0 if literal_type2_avg else soffset                                             # :355-368, :388-435 leave soffset out
        pil = 0
        re = k0
        P = lambda i: pilot[i] if i < len(pilot) else (0, 0)

        def prb(first):
            nonlocal pil, re
            ch0 = c32_mul_shift(P(pil), rxdataF[(soffset if first else so) + nushift + re], 15)
            pil += 1
            re = (re + 1) % N
            t = c32_mul_shift(P(pil), rxdataF[so + nushift + re], 15)
            ch0 = (ch0[0] + t[0], ch0[1] + t[1])
            pil += 1
            re = (re + 5) % N
            t = c32_mul_shift(P(pil), rxdataF[so + nushift + re], 15)
            ch0 = (ch0[0] + t[0], ch0[1] + t[1])
            if not (first and literal_type2_avg):                                            # :361-366: the first PRB has no pil++ here
                pil += 1
            re = (re + 1) % N
            t = c32_mul_shift(P(pil), rxdataF[so + nushift + re], 15)
            ch0 = (ch0[0] + t[0], ch0[1] + t[1])
            pil += 1
            re = (re + 5) % N
            return c16_div(ch0, 4)
        ch = prb(True)
        for _ in range(12):
            ul_ch[at] = ch
            at += 1
        for pilot_cnt in range(4, 4 * (nb_rb - 1), 4):                                       # :386
            ch = prb(False)
            for _ in range(12):
                ul_ch[at] = ch
                at += 1
        ch = prb(False)                                                                      # :423, also when nb_rb = 1
        for _ in range(12):
            ul_ch[at] = ch
            at += 1
    return ul_ch
