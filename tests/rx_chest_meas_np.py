"""A literal Python restatement of what the reference's PUSCH channel estimation measures besides the estimates -- max_ch and nvar --
and of nr_chest_time_domain_avg, loop by loop, for the tests to compare csrc/nr_chest.h and csrc/tb_rx_chest_meas.hip against.
Line numbers: openair1/PHY/NR_ESTIMATION/nr_ul_channel_estimation.c unless another file is named.  The loops are this file's own
(ul_ls_est and ul_ch are formed here, nothing calls the library); the primitives -- casts, products, the filter step, the pilots,
the delay tables -- are rx_chest_np.py's.  Values are Python ints; a c16 is a pair (r, i).

`mis` names misreadings of the reference, one at a time, for tests/test_rx_chest_meas_host.py to show that its cases notice each:
what a result would be if the implementation had read the text that way."""
import rx_chest_np as R

MISREADINGS = ("max_after_cast", "avg_edges", "noise32", "sat_sub", "t2_twice", "t2_none", "nest_per_antenna", "div_per_antenna",
               "div_after_sum", "div_dmrs", "max_per_layer")
AVG_MISREADINGS = ("wide_sum", "shift3", "round_div", "reverse_order")


def c16sub(a, b, mis=()):                     # tools_defs.h:186-191: the difference is cast, it wraps
    if "sat_sub" in mis:
        return (R.sat16(a[0] - b[0]), R.sat16(a[1] - b[1]))
    return (R.s16(a[0] - b[0]), R.s16(a[1] - b[1]))


def c16amp2(a):                               # tools_defs.h:182-184: uint32
    return (a[0] * a[0] + a[1] * a[1]) & 0xffffffff


def c16addShift(a, b, s):                     # tools_defs.h:200-205
    return (R.s16((a[0] + b[0]) >> s), R.s16((a[1] + b[1]) >> s))


def estimation_call(rx_ants, soffset, N, k0, nb_rb, p, dmrs_type, chest_freq, c_init, re_offset, est_delays, max_ch, mis=()):
    """One call of nr_pusch_channel_estimation (:67-473): one DMRS symbol, port p, all antennas.  rx_ants[aarx] = that antenna's
    buffer as a list of c16 pairs, est_delays[aarx] = what nr_est_delay would have found (:194, :278), max_ch = *max_ch as carried
    in.  Returns (max_ch, nvar_tmp, noise_amp2, nest_count, ul_ch per antenna: 12 nb_rb pairs)."""
    nushift = (p >> 1) & 1                                                                   # :89
    nb_dmrs = 6 if dmrs_type == 0 else 4
    pilot = R.pusch_dmrs_rx(c_init, p, nb_rb, re_offset, dmrs_type)                          # :114-122
    nest_count = 0                                                                           # :148
    noise_amp2 = 0                                                                           # :149, uint64_t
    per_antenna = []                                                                         # (noise, nest) of each antenna, for `mis`
    out = []
    for aarx, rxdataF in enumerate(rx_ants):                                                 # :155
        noise0, nest0 = noise_amp2, nest_count
        ul_ch = [(0, 0)] * (N + 32)                                                          # :159
        ul_ls_est = [(0, 0)] * (N + 32)                                                      # :150-151
        at = 0
        if dmrs_type == 0 and chest_freq == 0:                                               # :167
            pil = 0
            pilot_cnt = 0
            delta = R.delta1[p]                                                              # :174
            for n in range(3 * nb_rb):                                                       # :176
                ch = (0, 0)                                                                  # c32_t
                for k_line in range(2):
                    re = (k0 + (n << 2) + (k_line << 1) + delta) % N                         # :181
                    t = R.c32_mul_shift(pilot[pil], rxdataF[soffset + re], 16)
                    ch = (t[0] + ch[0], t[1] + ch[1])                                        # :182
                    pil += 1
                ch16 = (R.s16(ch[0]), R.s16(ch[1]))                                          # :186
                m = ch16 if "max_after_cast" in mis else ch
                max_ch = max(max_ch, max(abs(m[0]), abs(m[1])))                              # :187: the int32 value
                for k in range(pilot_cnt << 1, (pilot_cnt << 1) + 4):                        # :188-190
                    ul_ls_est[k] = ch16
                pilot_cnt += 2
            tab = R.delay_table_row(N, est_delays[aarx])                                     # :195-196
            pilot_cnt = 0
            for n in range(3 * nb_rb):                                                       # :203
                for k_line in range(2):
                    k = pilot_cnt << 1
                    ch16 = R.c16_mul_shift(ul_ls_est[k], tab[k], 8)                          # :210
                    if pilot_cnt == 0:
                        R.multadd_vect_real_complex(R.filt16_ul_p0, ch16, ul_ch, at)
                    elif pilot_cnt == 1 or pilot_cnt == 2:
                        R.multadd_vect_real_complex(R.filt16_ul_p1p2, ch16, ul_ch, at)
                    elif pilot_cnt == 6 * nb_rb - 1:
                        R.multadd_vect_real_complex(R.filt16_ul_last, ch16, ul_ch, at)
                    else:
                        R.multadd_vect_real_complex(R.filt16_ul_middle, ch16, ul_ch, at)
                        if pilot_cnt % 2 == 0:
                            at += 4                                                          # :228
                    pilot_cnt += 1
            inv = R.delay_table_row(N, -est_delays[aarx])                                    # :239-240
            pilot_cnt = 0
            for n in range(3 * nb_rb):                                                       # :241
                for k_line in range(2):
                    k = pilot_cnt << 1
                    ul_ch[k] = R.c16_mul_shift(ul_ch[k], inv[k], 8)                          # :244
                    ul_ch[k + 1] = R.c16_mul_shift(ul_ch[k + 1], inv[k + 1], 8)              # :245
                    noise_amp2 += c16amp2(c16sub(ul_ls_est[k], ul_ch[k], mis))               # :246
                    noise_amp2 += c16amp2(c16sub(ul_ls_est[k + 1], ul_ch[k + 1], mis))       # :247
                    pilot_cnt += 1
                    nest_count += 2                                                          # :255
        elif dmrs_type == 1 and chest_freq == 0:                                             # :259
            pil = 0
            rx = soffset + nushift                                                           # :262
            for n in range(0, nb_rb * 12, 6):                                                # :263
                ch0 = R.c16_mul_shift(pilot[pil], rxdataF[rx + (k0 + n) % N], 15)            # :264
                pil += 1
                ch1 = R.c16_mul_shift(pilot[pil], rxdataF[rx + (k0 + n + 1) % N], 15)        # :266
                pil += 1
                ch = c16addShift(ch0, ch1, 1)                                                # :268
                max_ch = max(max_ch, max(abs(ch[0]), abs(ch[1])))                            # :269
                yr = [R.s16(((ch[0] * x) >> 16) << 2) for x in R.filt8_rep4]                 # :270, as rx_chest_np.py
                yi = [R.s16(((ch[1] * x) >> 16) << 2) for x in R.filt8_rep4]
                for j in range(4):
                    y = ul_ls_est[n + j]
                    y = (R.sat16(y[0] + yr[j]), R.sat16(y[1] + yi[j]))
                    ul_ls_est[n + j] = (R.sat16(y[0] + yr[4 + j]), R.sat16(y[1] + yi[4 + j]))
                ul_ls_est[n + 4] = ch                                                        # :271
                ul_ls_est[n + 5] = ch                                                        # :272
                times = 2 if "t2_twice" in mis else (0 if "t2_none" in mis and n % 4 == 2 else 1)
                noise_amp2 += times * c16amp2(c16sub(ch0, ch, mis))                          # :273
                nest_count += 1                                                              # :274
            tab = R.delay_table_row(N, -est_delays[aarx])                                    # :279-280
            for n in range(nb_rb * 12):
                ul_ch[n] = R.c16_mul_shift(ul_ls_est[n], tab[n % 6], 8)                      # :282
        else:                                                                                # :287 (type 1), :344 (type 2): NO_INTERP
            rxF = soffset + nushift
            state = {"pil": 0, "re": k0}

            def prb():
                c = (0, 0)
                if dmrs_type == 0:                                                           # :45-65
                    for _ in range(6):
                        t = R.c32_mul_shift(pilot[state["pil"]], rxdataF[rxF + state["re"]], 15)
                        c = (t[0] + c[0], t[1] + c[1])
                        state["pil"] += 1
                        state["re"] = (state["re"] + 2) % N
                    return R.c16_div(c, 6)
                # :386-404 as every PRB but the first is written, with soffset (this project's form of TYPE2_AVG: every PRB
                # four pilots of its own, every read relative to the symbol)
                for step in (1, 5, 1, 5):
                    t = R.c32_mul_shift(pilot[state["pil"]], rxdataF[rxF + state["re"]], 15)
                    c = (t[0] + c[0], t[1] + c[1])
                    state["pil"] += 1
                    state["re"] = (state["re"] + step) % N
                return R.c16_div(c, 4)
            ch = prb()                                                                       # :295 / :350-373: the first PRB, no max_ch
            if "avg_edges" in mis:
                max_ch = max(max_ch, max(abs(ch[0]), abs(ch[1])))
            for _ in range(12):
                ul_ch[at] = ch
                at += 1
            for pilot_cnt in range(nb_dmrs, nb_dmrs * (nb_rb - 1), nb_dmrs):                 # :309 / :386
                ch = prb()
                max_ch = max(max_ch, max(abs(ch[0]), abs(ch[1])))                            # :311 / :405
                for _ in range(12):
                    ul_ch[at] = ch
                    at += 1
            if nb_rb > 1:                                                                    # :330 / :423: the last PRB, no max_ch
                ch = prb()                                                                   # (with one PRB the reference writes it
                if "avg_edges" in mis:                                                       # behind the allocation: not kept)
                    max_ch = max(max_ch, max(abs(ch[0]), abs(ch[1])))
                for _ in range(12):
                    ul_ch[at] = ch
                    at += 1
        per_antenna.append((noise_amp2 - noise0, nest_count - nest0))
        out.append(ul_ch[:12 * nb_rb])
    if "noise32" in mis:
        noise_amp2 &= 0xffffffff
    nvar_tmp = 0                                                                             # nr_ulsch_demodulation.c:1481
    if "nest_per_antenna" in mis and per_antenna[0][1] > 0:
        nvar_tmp = (noise_amp2 // per_antenna[0][1]) & 0xffffffff
    elif "div_per_antenna" in mis:
        nvar_tmp = sum(a // b for a, b in per_antenna if b > 0) & 0xffffffff
    elif nest_count > 0:                                                                     # :468-469
        nvar_tmp = (noise_amp2 // nest_count) & 0xffffffff
    return max_ch, nvar_tmp, noise_amp2, nest_count, out


def pdu_measurements(calls, nr_of_symbols, nrOfLayers, nb_antennas_rx, n_dmrs=None, mis=()):
    """The estimation loop of nr_rx_pusch_tp (nr_ulsch_demodulation.c:1470-1524) for one PDU.  calls = the PDU's calls in any
    order, each a dict of estimation_call's arguments but max_ch, with "layer" besides.  Returns (max_ch, nvar, ul_ch per call)."""
    max_ch = 0                                                                               # :1470
    nvar = 0                                                                                 # :1471, uint32_t
    layer_max, noise_sum, nest_sum, ch = {}, 0, 0, []
    for c in calls:                                                                          # :1472-1492
        args = {k: v for k, v in c.items() if k != "layer"}
        if "max_per_layer" in mis:
            m, nvar_tmp, noise, nest, ul_ch = estimation_call(max_ch=layer_max.get(c["layer"], 0), mis=mis, **args)
            layer_max[c["layer"]] = m
            max_ch = layer_max.get(0, 0)
        else:
            max_ch, nvar_tmp, noise, nest, ul_ch = estimation_call(max_ch=max_ch, mis=mis, **args)
        nvar = (nvar + nvar_tmp) & 0xffffffff                                                # :1491
        noise_sum, nest_sum = noise_sum + noise, nest_sum + nest
        ch.append(ul_ch)
    if "div_after_sum" in mis:
        nvar = (noise_sum // nest_sum) & 0xffffffff if nest_sum else 0
    div = (n_dmrs if "div_dmrs" in mis else nr_of_symbols) * nrOfLayers * nb_antennas_rx
    nvar //= div                                                                             # :1524: all symbols of the allocation
    return max_ch, nvar, ch


def chest_time_domain_avg(symbols, mis=()):
    """nr_chest_time_domain_avg (openair1/PHY/NR_REFSIG/dmrs_nr.c:343-417) for one plane: symbols = the 12 num_rbs c16 of each DMRS
    symbol in symbol order, as lists of pairs.  Returns the first symbol's entries as the function leaves them."""
    n = len(symbols)
    assert 1 <= n <= 4                                                                       # :415
    first = [tuple(c) for c in symbols[0]]
    later = symbols[1:][::-1] if "reverse_order" in mis else symbols[1:]
    for sym in later:                                                                        # :358-370
        if "wide_sum" in mis:
            first = [(a[0] + b[0], a[1] + b[1]) for a, b in zip(first, sym)]
        else:
            first = [(R.sat16(a[0] + b[0]), R.sat16(a[1] + b[1])) for a, b in zip(first, sym)]   # adds_epi16
    if n == 2:
        return [(a[0] >> 1, a[1] >> 1) for a in first]                                       # :372-378 srai_epi16
    if n == 4:
        return [(a[0] >> 2, a[1] >> 2) for a in first]                                       # :379-385
    if n == 3:                                                                               # :386-414: int16 /= 3
        if "shift3" in mis:
            q = lambda x: (x * 10923) >> 15
        elif "round_div" in mis:
            q = lambda x: (abs(x) + 1) // 3 * (1 if x >= 0 else -1)
        else:
            q = lambda x: abs(x) // 3 * (1 if x >= 0 else -1)                                # C: towards zero
        return [(q(a[0]), q(a[1])) for a in first]
    return first
