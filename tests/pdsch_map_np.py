"""A literal Python restatement of the reference's PDSCH resource mapping and unit-precoding copy, loop by loop, for the tests to
compare csrc/nr_pdsch_map.h against.  Line numbers: openair1/PHY/NR_TRANSPORT/nr_dlsch.c unless another file is named.  It keeps
the running k, n, k_prime, dmrs_idx and m of the DMRS branch, the two-piece four-RE loop with its scalar tail of the branch without
DMRS, and allowed_xlsch_re_in_dmrs_symbol as written.  Two flags switch the reference's two defects off: literal_tail=False gives
the scalar tail the final shift of mulhrs, literal_allowed=False takes diff = 0 at the allocation's first subcarrier.  PTRS is left
out (pduBitmap & 1 = 0), precoding is unit (prg_size = 0: pmi = 0, one RB per step).  The Gold sequence is rx_chest_np's plain
bit-by-bit LFSR, independent of csrc/nr_gold.h.  Values are Python ints; a c16 is a pair (r, i)."""
from rx_chest_np import gold_bits, s16

# nr_sch_dmrs.c:37-57: ap, CDM group, delta, Wf(0), Wf(1), Wt(0), Wt(1)
pdsch_dmrs_1 = [[0, 0, 0, 1, 1, 1, 1], [1, 0, 0, 1, -1, 1, 1], [2, 1, 1, 1, 1, 1, 1], [3, 1, 1, 1, -1, 1, 1],
                [4, 0, 0, 1, 1, 1, -1], [5, 0, 0, 1, -1, 1, -1], [6, 1, 1, 1, 1, 1, -1], [7, 1, 1, 1, -1, 1, -1]]
pdsch_dmrs_2 = [[0, 0, 0, 1, 1, 1, 1], [1, 0, 0, 1, -1, 1, 1], [2, 1, 2, 1, 1, 1, 1], [3, 1, 2, 1, -1, 1, 1], [4, 2, 4, 1, 1, 1, 1],
                [5, 2, 4, 1, -1, 1, 1], [6, 0, 0, 1, 1, 1, -1], [7, 0, 0, 1, -1, 1, -1], [8, 1, 2, 1, 1, 1, -1], [9, 1, 2, 1, -1, 1, -1],
                [10, 2, 4, 1, 1, 1, -1], [11, 2, 4, 1, -1, 1, -1]]
SI_RNTI = 0xffff
QPSK_AMP = 16384                              # (short)(32768 * 0.70711f * 0.70711f), nr_gen_mod_table.c:46-47


def table(dmrs_type):
    return pdsch_dmrs_1 if dmrs_type == 0 else pdsch_dmrs_2


def get_Wt(ap, dmrs_type):                    # nr_sch_dmrs.c:68-72
    return table(dmrs_type)[ap][5:7]


def get_Wf(ap, dmrs_type):                    # :74-78
    return table(dmrs_type)[ap][3:5]


def get_delta(ap, dmrs_type):                 # :80-82
    return table(dmrs_type)[ap][2]


def get_dmrs_freq_idx(n, k_prime, delta, dmrs_type):   # :84-87
    return 6 * n + k_prime + delta if dmrs_type else (n << 2) + (k_prime << 1) + delta


def get_l0(dl_dmrs_symb_pos):                 # :89-98
    mask, l0 = dl_dmrs_symb_pos, 0
    while l0 < 14:
        if mask & 1:
            break
        mask >>= 1
        l0 += 1
    return l0


def get_dmrs_port(nl, dmrs_ports):            # common/utils/nr/nr_common.c:494-511
    if dmrs_ports == 0:
        return 0
    found = -1
    for i in range(12):
        if (dmrs_ports >> i) & 1:
            found += 1
            if found == nl:
                return i
    raise AssertionError("No dmrs port corresponding to layer %d found" % nl)


def c_init_pdsch(slot, symb, nid, nscid):     # nr_init_pdsch_dmrs, nr_gold.c:87-88
    return ((1 << 17) * (14 * slot + symb + 1) * ((nid << 1) + 1) + ((nid << 1) + nscid)) % (1 << 31)


def allowed_xlsch_re_in_dmrs_symbol(k, start_sc, ofdm_symbol_size, num_cdm_no_data, dmrs_type, literal=True):   # dmrs_nr.c:37-62
    if k > start_sc or (not literal and k == start_sc):
        diff = k - start_sc
    else:
        diff = (ofdm_symbol_size - start_sc) + k
    for i in range(num_cdm_no_data):
        if dmrs_type == 0:
            if diff % 2 == i:
                return 0
        else:
            delta = i << 1
            if diff % 6 == delta or diff % 6 == delta + 1:
                return 0
    return 1


def mod_dmrs(c_init, n):
    """nr_modulation of the symbol's Gold words with Qm = 2 (:271-274): entry s from bits 2s and 2s + 1"""
    g = gold_bits(c_init, 2 * n + 2)
    return [((1 - 2 * g[2 * s]) * QPSK_AMP, (1 - 2 * g[2 * s + 1]) * QPSK_AMP) for s in range(n)]


def c16_mul_real_shift(a, b, shift):          # tools_defs.h:214-217
    return (s16((a[0] * b) >> shift), s16((a[1] * b) >> shift))


def mulhrs(a, b):                             # simde_mm_mulhrs_epi16
    return s16((((a * b) >> 14) + 1) >> 1)


def start_subcarrier(p):                      # :208-210
    start_sc = p["first_carrier_offset"] + (p["rb_start"] + p["bwp_start"]) * 12
    if start_sc >= p["fft_size"]:
        start_sc -= p["fft_size"]
    return start_sc


def symbol_params(p):
    """What the loops derive per OFDM symbol, for the tests of the descriptor builder: a list of dicts in symbol order with dmrs,
    l_prime, dmrs_idx (the first sequence symbol) and c_init."""
    out = []
    l_prime, l_overline = 0, get_l0(p["dl_dmrs_symb_pos"])                                   # :229-230
    typ = p["dmrs_config_type"]
    for l_symbol in range(p["start_symbol"], p["start_symbol"] + p["nr_of_symbols"]):
        d = dict(symbol=l_symbol, dmrs=bool(p["dl_dmrs_symb_pos"] & (1 << l_symbol)))
        if d["dmrs"]:
            dmrs_idx = p["rb_start"]                                                         # :260
            if p["rnti"] != SI_RNTI:
                dmrs_idx += p["bwp_start"]
            dmrs_idx *= 6 if typ == 0 else 4
            if l_symbol == l_overline + 1:                                                   # :264-269
                l_prime = 1
            elif l_symbol > l_overline + 1:
                l_overline = l_symbol
                l_prime = 0
            d.update(l_prime=l_prime, dmrs_idx=dmrs_idx, c_init=c_init_pdsch(p["slot"], l_symbol, p["dl_dmrs_scrambling_id"], p["scid"]))
        out.append(d)
    return out


def pdsch_resource_mapping(p, tx_layers, n_tx, literal_tail=True, literal_allowed=True, fill=None):
    """p: Nl, dmrs_config_type, num_dmrs_cdm_grps_no_data, dmrs_ports, scid, dl_dmrs_scrambling_id, slot, rnti, amp, fft_size,
    first_carrier_offset, bwp_start, rb_start, rb_size, start_symbol, nr_of_symbols, dl_dmrs_symb_pos.  tx_layers[layer] = list of
    (r, i).  Returns (txdataF[ant][symbol][k] with `fill` where nothing was written, m per layer): the slot of n_tx antennas and
    how many entries of its plane each layer consumed."""
    N, amp, typ = p["fft_size"], p["amp"], p["dmrs_config_type"]
    start_sc = start_subcarrier(p)
    n_re = p["rb_size"] * 12
    precoding = [[[None] * N for _ in range(14)] for _ in range(p["Nl"])]
    consumed = []
    for layer in range(p["Nl"]):                                                             # :221
        dmrs_port = get_dmrs_port(layer, p["dmrs_ports"])
        Wt, Wf, delta = get_Wt(dmrs_port, typ), get_Wf(dmrs_port, typ), get_delta(dmrs_port, typ)
        l_prime, l_overline = 0, get_l0(p["dl_dmrs_symb_pos"])
        m, dmrs_idx = 0, 0
        txl = tx_layers[layer]
        for l_symbol in range(p["start_symbol"], p["start_symbol"] + p["nr_of_symbols"]):     # :252
            k_prime, n = 0, 0
            is_dmrs = bool(p["dl_dmrs_symb_pos"] & (1 << l_symbol))
            out = precoding[layer][l_symbol]
            if is_dmrs:                                                                      # :256-274
                dmrs_idx = p["rb_start"]
                if p["rnti"] != SI_RNTI:
                    dmrs_idx += p["bwp_start"]
                dmrs_idx *= 6 if typ == 0 else 4
                if l_symbol == l_overline + 1:
                    l_prime = 1
                elif l_symbol > l_overline + 1:
                    l_overline = l_symbol
                    l_prime = 0
                mod = mod_dmrs(c_init_pdsch(p["slot"], l_symbol, p["dl_dmrs_scrambling_id"], p["scid"]), dmrs_idx + n_re)
            k = start_sc                                                                     # :299
            if is_dmrs:
                for _ in range(n_re):                                                        # :302
                    if k == (start_sc + get_dmrs_freq_idx(n, k_prime, delta, typ)) % N:      # :316-318
                        out[k] = c16_mul_real_shift(mod[dmrs_idx], Wt[l_prime] * Wf[k_prime] * amp, 15)
                        dmrs_idx += 1
                        k_prime += 1
                        k_prime &= 1
                        n += 0 if k_prime else 1
                    elif allowed_xlsch_re_in_dmrs_symbol(k, start_sc, N, p["num_dmrs_cdm_grps_no_data"], typ, literal_allowed):   # :354-359
                        out[k] = c16_mul_real_shift(txl[m], amp, 15)
                        m += 1
                    else:
                        out[k] = (0, 0)                                                      # :372
                    k += 1
                    if k >= N:
                        k -= N
            else:                                                                            # :377-471
                upper_limit, remaining_re = n_re, 0
                if start_sc + upper_limit > N:
                    remaining_re = upper_limit + start_sc - N
                    upper_limit = N - start_sc
                for base, length in ((start_sc, upper_limit), (0, remaining_re)):
                    if length <= 0:
                        continue
                    for i in range(length >> 2):                                             # :410-412, :441-443: four c16 at a time
                        for u in range(4):
                            x = txl[m + 4 * i + u]
                            out[base + 4 * i + u] = (mulhrs(amp, x[0]), mulhrs(amp, x[1]))
                    for i in range((length >> 2) << 2, length):                              # :428-435, :460-467
                        x = txl[m + i]
                        if literal_tail:
                            out[base + i] = (s16(((x[0] * amp) >> 14) + 1), s16(((x[1] * amp) >> 14) + 1))
                        else:
                            out[base + i] = (mulhrs(amp, x[0]), mulhrs(amp, x[1]))
                    m += length
        consumed.append(m)
    # unit precoding (:486-535): RB by RB, split where an RB crosses the end of the symbol
    tx = [[[fill] * N for _ in range(14)] for _ in range(n_tx)]
    for ant in range(n_tx):
        for l_symbol in range(p["start_symbol"], p["start_symbol"] + p["nr_of_symbols"]):
            sub = start_sc
            for _ in range(p["rb_size"]):
                re_cnt = 12
                pieces = [(sub, re_cnt)] if sub + re_cnt <= N else [(sub, N - sub), (0, re_cnt - (N - sub))]
                for at, cnt in pieces:
                    for q in range(at, at + cnt):
                        tx[ant][l_symbol][q] = precoding[ant][l_symbol][q] if ant < p["Nl"] else (0, 0)
                sub += re_cnt
                if sub >= N:
                    sub -= N
    return tx, consumed
