"""numpy restatement of the RB extraction of the single-layer PUSCH receiver, written from the reference's lines
(openair1/PHY/NR_TRANSPORT/nr_ulsch_demodulation.c:279-380 nr_ulsch_extract_rbs, :417-431 get_nb_re_pusch, :1584-1589 the
measurement symbol, :1654-1665 the llr_offset loop; :1460, :1472-1478, :1527-1537 and :1402-1408 the writers of
pusch_vars->dmrs_symbol, with :1654-1666 which decides whether a symbol gets a job at all, dmrs_symbol_rule below) -- not from csrc/nr_rx_grid.h.  The branches and loops are kept as they stand:
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


INVALID_VALUE = 255


def get_next_dmrs_symbol_in_slot(ul_dmrs_symb_pos, counter, end_symbol):
    """openair1/PHY/NR_REFSIG/dmrs_nr.c:299-307"""
    symbol = counter
    while symbol < end_symbol:
        if (ul_dmrs_symb_pos >> symbol) & 0x01:
            return symbol
        symbol += 1
    return -1


def dmrs_symbol_rule(pdu, chest_time, job_for_every_symbol=False):
    """Whose estimates each symbol reads: (the dmrs_symbol the level reads at :1606, {symbol: the dmrs_symbol its inner_rx reads at
    :1294, for the symbols that reach inner_rx}), restated from pusch_vars->dmrs_symbol's three writers in nr_rx_pusch_tp and the
    one in nr_pusch_symbol_processing.  pdu: ul_dmrs_symb_pos, start_symbol_index, nr_of_symbols and what get_nb_re_pusch reads.
    num_pusch_symbols_per_thread = 1 (nr-gnb.c:372, ulsim.c:554; symbol_loop below assumes it too): a job covers one symbol and is
    created only when that symbol has REs (:1666), so a DMRS symbol without REs -- type 1 with two CDM groups without data -- has
    no job, :1408 never runs for it, and the symbols behind it keep the DMRS symbol they had.  The jobs run in order, one after
    the other: the reference's result with one job in flight (its jobs share pusch_vars->dmrs_symbol).  INVALID_VALUE stays where
    no DMRS symbol lies in the allocation.
    job_for_every_symbol = True is NOT the reference: the gate at :1666 lifted, so that every DMRS symbol moves dmrs_symbol whether
    it has REs or not.  It is what the library's dmrs_symbol = 255 does; the two differ for two CDM groups alone."""
    ul_dmrs_symb_pos, start_symbol_index, nr_of_symbols = pdu["ul_dmrs_symb_pos"], pdu["start_symbol_index"], pdu["nr_of_symbols"]
    dmrs_symbol = INVALID_VALUE                                                                                     # :1460
    symbol = start_symbol_index
    while symbol < start_symbol_index + nr_of_symbols:                                                              # :1472
        dmrs_symbol_flag = (ul_dmrs_symb_pos >> symbol) & 0x01                                                      # :1473
        if dmrs_symbol_flag == 1:                                                                                   # :1476
            if dmrs_symbol == INVALID_VALUE:                                                                        # :1477
                dmrs_symbol = symbol                                                                                # :1478
        symbol += 1
    if chest_time == 1:                                                                                             # :1527
        # :1535-1537, as called: end_symbol = nr_of_symbols, not start_symbol_index + nr_of_symbols; the -1 lands in a uint8_t
        dmrs_symbol = get_next_dmrs_symbol_in_slot(ul_dmrs_symb_pos, start_symbol_index, nr_of_symbols) & 0xff
    level = dmrs_symbol                                                                                             # :1606
    numSymbols = 1                                                                                                  # :1652
    read, ul_valid_re_per_slot = {}, {}
    symbol = start_symbol_index
    while symbol < start_symbol_index + nr_of_symbols:                                                              # :1654-1656
        total_res = 0                                                                                               # :1658
        for s in range(numSymbols):                                                                                 # :1659
            ul_valid_re_per_slot[symbol + s] = get_nb_re_pusch(pdu, symbol + s)                                     # :1660
            total_res += ul_valid_re_per_slot[symbol + s]                                                           # :1664
        if total_res > 0 or job_for_every_symbol:                                                                   # :1666
            startSymbol = symbol                                                                                    # :1676
            job_symbol = startSymbol
            while job_symbol < startSymbol + numSymbols:                                                            # :1402
                dmrs_symbol_flag = (ul_dmrs_symb_pos >> job_symbol) & 0x01                                          # :1403
                if dmrs_symbol_flag == 1:                                                                           # :1404
                    dmrs_symbol = job_symbol                                                                        # :1408
                if ul_valid_re_per_slot[job_symbol] != 0:                                                           # :1411-1412
                    read[job_symbol] = dmrs_symbol                                                                  # :1414 -> :1294
                job_symbol += 1
        symbol += numSymbols
    return level, read


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
