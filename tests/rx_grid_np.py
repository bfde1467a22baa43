"""numpy restatement of the RB extraction of the single-layer PUSCH receiver, written from the reference's lines
(openair1/PHY/NR_TRANSPORT/nr_ulsch_demodulation.c:279-380 nr_ulsch_extract_rbs, :417-431 get_nb_re_pusch, :1584-1589 the
measurement symbol, :1654-1665 the llr_offset loop) -- not from csrc/nr_rx_grid.h.  The branches and loops are kept as they stand:
the three cases, the one-piece and the two-piece form of each, `<` at :317 / :346 against `<=` at :302, and idx2 carrying the
channel index into the second piece.  rxdataF = int16 [>= rxoffset + N, 2] of one antenna, chF = int16 [.., 2]."""
import numpy as np

NR_NB_SC_PER_RB = 12
pusch_dmrs_type1, pusch_dmrs_type2 = 0, 1
SYMBOLS_PER_SLOT = 14


def extract_rbs(rxdataF, chF, rxoffset, choffset, is_dmrs_symbol, pdu, fp, fix_352=False):
    """pdu: rb_start, bwp_start, rb_size, dmrs_config_type; fp: first_carrier_offset, ofdm_symbol_size.  Returns (rxFext, chFext)
    as lists grown by the `*rxF_ext++ =` statements.  fix_352 adds start_re where the one-piece type-2 branch reads rxF[idx]."""
    delta = 0
    N = fp["ofdm_symbol_size"]
    start_re = (fp["first_carrier_offset"] + (pdu["rb_start"] + pdu["bwp_start"]) * NR_NB_SC_PER_RB) % N          # :292
    nb_re_pusch = NR_NB_SC_PER_RB * pdu["rb_size"]
    rxF = rxdataF[rxoffset:]
    ul_ch0 = chF[choffset:]
    rxF_ext, ul_ch0_ext = [], []
    if is_dmrs_symbol == 0:
        if start_re + nb_re_pusch <= N:                                                                             # :302
            rxF_ext.extend(rxF[start_re:start_re + nb_re_pusch])
        else:
            neg_length = N - start_re
            pos_length = nb_re_pusch - neg_length
            rxF_ext.extend(rxF[start_re:start_re + neg_length])
            rxF_ext.extend(rxF[0:pos_length])
        ul_ch0_ext.extend(ul_ch0[0:nb_re_pusch])                                                                    # :311
    elif pdu["dmrs_config_type"] == pusch_dmrs_type1:
        rxF32 = rxF[start_re:]
        if start_re + nb_re_pusch < N:                                                                              # :317
            idx = 1 - delta
            while idx < nb_re_pusch:
                rxF_ext.append(rxF32[idx])
                ul_ch0_ext.append(ul_ch0[idx])
                idx += 2
        else:
            neg_length = N - start_re
            pos_length = nb_re_pusch - neg_length
            idx = 1 - delta
            while idx < neg_length:
                rxF_ext.append(rxF32[idx])
                ul_ch0_ext.append(ul_ch0[idx])
                idx += 2
            rxF32 = rxF
            idx2 = idx
            idx = 1 - delta
            while idx < pos_length:
                rxF_ext.append(rxF32[idx])
                ul_ch0_ext.append(ul_ch0[idx2])
                idx += 2
                idx2 += 2
    elif pdu["dmrs_config_type"] == pusch_dmrs_type2:
        if start_re + nb_re_pusch < N:                                                                              # :346
            for idx in range(nb_re_pusch):
                if idx % 6 == 2 * delta or idx % 6 == 2 * delta + 1:
                    continue
                rxF_ext.append(rxF[start_re + idx] if fix_352 else rxF[idx])                                        # :352
                ul_ch0_ext.append(ul_ch0[idx])
        else:
            neg_length = N - start_re
            pos_length = nb_re_pusch - neg_length
            rxF64 = rxF[start_re:]
            idx = 0
            while idx < neg_length:
                if not (idx % 6 == 2 * delta or idx % 6 == 2 * delta + 1):
                    rxF_ext.append(rxF64[idx])
                    ul_ch0_ext.append(ul_ch0[idx])
                idx += 1
            rxF64 = rxF
            idx2 = idx
            idx = 0
            while idx < pos_length:
                if not (idx % 6 == 2 * delta or idx % 6 == 2 * delta + 1):
                    rxF_ext.append(rxF64[idx])
                    ul_ch0_ext.append(ul_ch0[idx2])
                idx += 1
                idx2 += 1
    as_arr = lambda v: np.array(v, np.int16).reshape(-1, 2)
    return as_arr(rxF_ext), as_arr(ul_ch0_ext)


def get_nb_re_pusch(pdu, symbol):
    """:417-431; raises where the reference asserts"""
    if (pdu["ul_dmrs_symb_pos"] >> symbol) & 1:
        if (pdu["ul_dmrs_symb_pos"] >> ((symbol + 1) % SYMBOLS_PER_SLOT)) & 1:
            raise AssertionError("Double DMRS configuration is not yet supported")
        if pdu["dmrs_config_type"] == 0:
            return pdu["rb_size"] * (12 - pdu["num_dmrs_cdm_grps_no_data"] * 6)
        return pdu["rb_size"] * (12 - pdu["num_dmrs_cdm_grps_no_data"] * 4)
    return pdu["rb_size"] * NR_NB_SC_PER_RB


def symbol_loop(pdu, Qm):
    """(meas_symbol, [(symbol, nb_re, llr_offset / Qm) for the symbols with REs]) as :1584-1589 and :1654-1665 give them
    (num_pusch_symbols_per_thread = 1)"""
    meas_symbol, first, last = -1, pdu["start_symbol_index"], pdu["start_symbol_index"] + pdu["nr_of_symbols"]
    for s in range(first, last):
        if get_nb_re_pusch(pdu, s) > 0:
            meas_symbol = s
            break
    valid, llr_offset, out = {}, {}, []
    for symbol in range(first, last):
        valid[symbol] = get_nb_re_pusch(pdu, symbol)
        llr_offset[symbol] = 0 if symbol == first else llr_offset[symbol - 1] + valid[symbol - 1] * Qm
        if valid[symbol] > 0:
            out.append((symbol, valid[symbol], llr_offset[symbol] // Qm))
    return meas_symbol, out
