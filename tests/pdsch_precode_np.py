"""A literal Python restatement of the reference's PDSCH precoding, for the tests to compare csrc/nr_pdsch_map.h's precoding against:
nr_layer_precoder_simd (openair1/PHY/MODULATION/nr_modulation.c:720-821) lane by lane on its 128-bit instruction sequence, the same
per RE in integer arithmetic, nr_layer_precoder_cm (:702-718, c16maddShift of openair1/PHY/TOOLS/tools_defs.h:226-231), and the RB
loop of nr_generate_pdsch (openair1/PHY/NR_TRANSPORT/nr_dlsch.c:486-589) with its rb_step pairing and its `<` against the symbol
size, which decides the path an RE takes.  The mapped layer grids come from pdsch_map_np.  Values are Python ints; a c16 is a pair
(r, i); a 128-bit register is a list of eight int16 lanes (or four int32 lanes).  A matrix is a dict with pm_idx, numLayers,
num_ant_ports and weights[layer][port] = (Re, Im); the reference's table is indexed by pmi - 1 (:540) and asserts that the entry
carries pm_idx = pmi, which the caller of precoding_loop arranges."""
from rx_chest_np import s16


def s32(v):
    return ((v + (1 << 31)) & 0xffffffff) - (1 << 31)


# ---- the SIMDe instructions the sequence uses ----
def mm_set1_epi32(c):                          # c = (r, i): the c16 as one 32-bit lane, r in the low half
    return [c[0], c[1]] * 4


def mm_madd_epi16(a, b):                       # eight int16 lanes each -> four int32 lanes; the one sum that can overflow wraps
    return [s32(a[2 * k] * b[2 * k] + a[2 * k + 1] * b[2 * k + 1]) for k in range(4)]


def mm_srai_epi32(a, n):
    return [v >> n for v in a]


def mm_slli_epi32(a, n):
    return [s32(v << n) for v in a]


def epi32_to_epi16(a):                         # the same register seen as eight int16 lanes, little endian
    out = []
    for v in a:
        out += [s16(v & 0xffff), s16((v >> 16) & 0xffff)]
    return out


def mm_blend_epi16(a, b, imm):                 # lane k from b where bit k of imm is set
    return [b[k] if (imm >> k) & 1 else a[k] for k in range(8)]


def mm_adds_epi16(a, b):
    return [max(-32768, min(32767, x + y)) for x, y in zip(a, b)]


def c16conj(w):                                # tools_defs.h: .i = -x.i, stored to an int16
    return (w[0], s16(-w[1]))


def c16swap(w):
    return (w[1], w[0])


def nr_layer_precoder_simd(n_layers, mapped, ant, pm, symbol, sc_offset, re_cnt, out):
    """:768-820, the 128-bit loop (the 256-bit loop of x86 is the same per lane).  mapped[layer][symbol][sc], out[sc] written"""
    sc = sc_offset
    re_cnt_align4 = re_cnt & ~3
    while sc < sc_offset + re_cnt_align4:
        y = [0] * 8                                                                          # :785
        for nl in range(n_layers):
            prec_weight = pm["weights"][nl][ant]
            x = [c for q in range(4) for c in mapped[nl][symbol][sc + q]]                    # :790
            w_c = mm_set1_epi32(c16conj(prec_weight))                                        # :793
            w_s = mm_set1_epi32(c16swap(prec_weight))                                        # :794
            reals = epi32_to_epi16(mm_srai_epi32(mm_madd_epi16(x, w_c), 15))                 # :797
            imags = epi32_to_epi16(mm_slli_epi32(mm_madd_epi16(x, w_s), 1))                  # :798
            produ = mm_blend_epi16(reals, imags, 0xAA)                                       # :807
            y = mm_adds_epi16(y, produ)                                                      # :810
        for q in range(4):                                                                   # :813
            out[sc + q] = (y[2 * q], y[2 * q + 1])
        sc += 4


def precode_re(xs, ws):
    """the same for one RE in integer arithmetic: xs[l], ws[l] = (r, i).  Returns ((r, i), clamped) with clamped = (a component was
    clamped from above, one from below)"""
    y, up, down = [0, 0], False, False
    for x, w in zip(xs, ws):
        nwi = s16(-w[1])
        t = (s16(s32(x[0] * w[0] + x[1] * nwi) >> 15), s16(s32(x[0] * w[1] + x[1] * w[0]) >> 15))
        for c in range(2):
            v = y[c] + t[c]
            up, down = up or v > 32767, down or v < -32768
            y[c] = max(-32768, min(32767, v))
    return (y[0], y[1]), (up, down)


def c16maddShift(a, b, c, shift):              # tools_defs.h:226-231; int arithmetic (the one sum that overflows in C wraps here)
    return (s16((s32(a[0] * b[0] - a[1] * b[1]) >> shift) + c[0]), s16((s32(a[0] * b[1] + a[1] * b[0]) >> shift) + c[1]))


def nr_layer_precoder_cm(n_layers, mapped, ap, pm, symbol, offset):   # :702-718
    y = (0, 0)
    for al in range(n_layers):
        y = c16maddShift(mapped[al][symbol][offset], pm["weights"][al][ap], y, 15)
    return y


def precoding_loop(p, mapped, n_tx, prg_size, prgs_list, pmi_pdu, fill=None):
    """nr_dlsch.c:486-589.  p as for pdsch_map_np (fft_size, rb_size, start_symbol, nr_of_symbols, Nl and what start_subcarrier
    reads); mapped[layer][symbol][sc] = txdataF_precoding; prgs_list = the pm_idx per PRG; pmi_pdu = the matrix table, entry pmi - 1
    carrying pm_idx = pmi.  Returns (tx[ant][symbol][sc], path[symbol][sc]): path is 'unit', 'simd' or 'cm', None where nothing was
    written."""
    from pdsch_map_np import start_subcarrier
    N, nl = p["fft_size"], p["Nl"]
    start_sc = start_subcarrier(p)
    tx = [[[fill] * N for _ in range(14)] for _ in range(n_tx)]
    path = [[None] * N for _ in range(14)]
    for ant in range(n_tx):                                                                  # :486
        for l_symbol in range(p["start_symbol"], p["start_symbol"] + p["nr_of_symbols"]):
            sub = start_sc
            out = tx[ant][l_symbol]
            rb = 0
            while rb < p["rb_size"]:                                                         # :491
                pmi = prgs_list[rb // prg_size] if prg_size > 0 else 0                       # :493-496
                pmi2 = prgs_list[(rb + 1) // prg_size] if rb < p["rb_size"] - 1 and prg_size > 0 else -1
                rb_step = 2 if pmi == pmi2 else 1                                            # :500
                re_cnt = 12 * rb_step
                if pmi == 0:                                                                 # :503-536
                    pieces = [(sub, re_cnt)] if sub + re_cnt <= N else [(sub, N - sub), (0, re_cnt - (N - sub))]
                    for at, cnt in pieces:
                        for q in range(at, at + cnt):
                            out[q] = mapped[ant][l_symbol][q] if ant < nl else (0, 0)
                            path[l_symbol][q] = "unit"
                    sub += re_cnt
                    if sub >= N:
                        sub -= N
                else:                                                                        # :537-584
                    assert n_tx > 1, "No precoding can be done with a single antenna port"
                    pm = pmi_pdu[pmi - 1]
                    assert pmi == pm["pm_idx"] and ant < pm["num_ant_ports"] and nl == pm["numLayers"]
                    if sub + re_cnt < N:                                                     # :547
                        nr_layer_precoder_simd(nl, mapped, ant, pm, l_symbol, sub, re_cnt, out)
                        for q in range(sub, sub + re_cnt):
                            path[l_symbol][q] = "simd"
                        sub += re_cnt
                    else:                                                                    # :560-583
                        for _ in range(re_cnt):
                            out[sub] = nr_layer_precoder_cm(nl, mapped, ant, pm, l_symbol, sub)
                            path[l_symbol][sub] = "cm"
                            sub += 1
                            if sub >= N:
                                sub -= N
                rb += rb_step
    return tx, path


def precode_all_simd(p, mapped, n_tx, prg_size, prgs_list, pmi_pdu, fill=None, per_re=False):
    """What the library defines: the write set and the PRGs of precoding_loop, but every RE of a PRG with pmi != 0 by the SIMD
    definition -- through nr_layer_precoder_simd on four REs of the allocation at a time (gathered around the wrap), or per_re through
    precode_re.  Returns (tx[ant][symbol][sc], (clamped from above, from below) anywhere)."""
    from pdsch_map_np import start_subcarrier
    N, nl = p["fft_size"], p["Nl"]
    start_sc = start_subcarrier(p)
    tx = [[[fill] * N for _ in range(14)] for _ in range(n_tx)]
    up = down = False
    for ant in range(n_tx):
        for l_symbol in range(p["start_symbol"], p["start_symbol"] + p["nr_of_symbols"]):
            out = tx[ant][l_symbol]
            for i0 in range(0, 12 * p["rb_size"], 4):
                pmi = prgs_list[(i0 // 12) // prg_size] if prg_size > 0 else 0
                ks = [(start_sc + i0 + q) % N for q in range(4)]
                if pmi == 0:
                    for k in ks:
                        out[k] = mapped[ant][l_symbol][k] if ant < nl else (0, 0)
                    continue
                pm = pmi_pdu[pmi - 1]
                assert pmi == pm["pm_idx"] and ant < pm["num_ant_ports"] and nl == pm["numLayers"]
                if per_re:
                    for k in ks:
                        out[k], (u, d) = precode_re([mapped[l][l_symbol][k] for l in range(nl)], [pm["weights"][l][ant] for l in range(nl)])
                        up, down = up or u, down or d
                else:
                    four = [{0: [mapped[l][l_symbol][k] for k in ks]} for l in range(nl)]     # the four REs as a symbol of their own
                    res = [None] * 4
                    nr_layer_precoder_simd(nl, four, ant, pm, 0, 0, 4, res)
                    for q, k in enumerate(ks):
                        out[k] = res[q]
    return tx, (up, down)
