"""The float64 PUSCH slot of ul_slot_np.py with several DMRS symbols and a channel that changes between them.  The channel of
ul_slot_np (a main tap per antenna, a weak second tap, the allocation across the grid's wrap) is multiplied by a complex factor
per OFDM symbol that is constant on each span the reference serves from one DMRS symbol -- [start, second DMRS symbol), [second,
third), ... -- and steps from span to span by a phase (`step` degrees) and a small gain change (`gain_step`, up on the odd spans):

    f[span i] = (1 + gain_step (i mod 2)) exp(i step pi / 180 . i)

The DMRS symbols go on the air with their span's factor; noise as in ul_slot_np.  On such a channel the rule of dmrs_symbol = 255
(every symbol reads the latest DMRS symbol at or before it: the reference's nr_ulsch_demodulation.c:1402-1408 wherever its DMRS
symbols have REs, rx_grid_np.dmrs_symbol_rule; with two CDM groups without data the library's own) is exactly
right and one symbol's estimates for the whole slot are exactly wrong; a smooth drift would blur the two.

The phase steps.  A wrong span's symbols are turned by `step` (or a multiple) against their estimates.  A constellation point at
angle a from the nearest decision boundary crosses it when turned by a: for 16QAM and above the corner and edge points next to the
axes' inner boundaries cross within 45 degrees (the 64QAM point 7 + 7i lies 45 degrees from both axes but only atan(1/7) = 8 degrees
from leaving its own cell), so 45 degrees puts the larger part of every wrong symbol's bits on the wrong side with full confidence;
QPSK / 16QAM sign bits cross at 45 degrees exactly, hence 60 there.  With three DMRS symbols the outer spans differ by 2 step.  The
variant that leaves the DMRS symbols alone on the previous span's estimates touches the fewest REs (6 or 8 of 12 subcarriers of one
or two symbols); the code rates are chosen so that even this no longer decodes, and test_ul_slot_tv_host.py asserts it.

CASES_CT1 are chest_time = 1 on a constant channel (factor 1): estimation, pusch_chest_time_avg over the three DMRS symbols, an
explicit alloc.dmrs_symbol = the first DMRS symbol, the receivers, decode."""
import numpy as np

import ul_slot_np as U

FOLLOW = 255                            # alloc.dmrs_symbol: NRLDPC_HIP_DMRS_SYMBOL_FOLLOW


def _tv(name, base, dmrs, step, gain_step, **over):
    """base: the case of ul_slot_np whose channel, mode, ports and modulation are taken; over: fields replaced"""
    return dict(U.CASE_BY_NAME[base], name=name, dmrs=tuple(dmrs), step=float(step), gain_step=gain_step, chest_time=0, **over)


CASES = [
    _tv("tv-1L-T1I", "1L-T1I-p0", (2, 11), 45, 0.05, rate=0.85),
    _tv("tv-1L-T2I-3dmrs", "1L-T2I-p1", (2, 7, 11), 45, 0.05, rate=0.85),
    _tv("tv-1L-T1A-dmrs0", "1L-T1A-p1", (0, 5, 10), 60, 0.05, rate=0.85),
    _tv("tv-1L-T1I-p2-cdm2", "1L-T1I-p2", (2, 11), 45, 0.05, rate=0.85),
    _tv("tv-2L-mmse", "2L-T1I", (2, 11), 45, 0.03, rate=0.75),
    _tv("tv-2L-ml16", "2L-T1I-ml16", (2, 11), 60, 0.03),
]
CASES_CT1 = [
    dict(_tv("ct1-1L-T1I", "1L-T1I-p0", (2, 7, 11), 0, 0.0), chest_time=1),
    dict(_tv("ct1-2L-mmse", "2L-T1I", (2, 7, 11), 0, 0.0, sigma=20.0), chest_time=1),
]
CASE_BY_NAME = {c["name"]: c for c in CASES + CASES_CT1}


span_of = U.span_of


def build_slot(m, case):
    """ul_slot_np.build_slot with the case's DMRS symbols and per-span factor; seg_tb / nvar_div besides: every descriptor is block
    0's, nvar_div = nr_of_symbols nrOfLayers n_rx"""
    c = case
    f_span = [(1.0 + c["gain_step"] * (i & 1)) * np.exp(1j * np.deg2rad(c["step"]) * i) for i in range(len(c["dmrs"]))]
    sl = U.build_slot(m, c, dmrs=c["dmrs"], f_span=f_span, rng_seed=9500 + c["seed"])
    return dict(sl, seg_tb=[0] * len(sl["csegs"]), nvar_div=[sl["alloc"]["nr_of_symbols"] * c["n_layers"] * c["n_rx"]])


_SLOTS = {}


def slot_of(m, name):
    """The case's slot, built once per session and shared; nobody writes to it."""
    if name not in _SLOTS:
        _SLOTS[name] = build_slot(m, CASE_BY_NAME[name])
        for v in _SLOTS[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _SLOTS[name]


def span_view(sl, i):
    """the slot as ul_slot_np's est_error / planes_of and test_ul_slot_host.bounds() see DMRS symbol i: that symbol's descriptor
    first, the true channel, g and e with the span's factor"""
    f = sl["f_span"][i]
    return dict(sl, csegs=[sl["csegs"][i]], h=sl["h"] * f, g=sl["g"] * f, e=sl["e"] * f)


def measured_host(m, sl):
    """(max_ch, nvar) of the block out of pusch_chest_meas_host per descriptor, as pusch_channel_estimation_meas forms them with
    every descriptor in block 0 and nvar_div = nr_of_symbols nrOfLayers n_rx"""
    mx, nv = 0, 0
    for s in sl["csegs"]:
        x, noise, nest = m.pusch_chest_meas_host(sl["rx"], sl["rx_stride"], sl["case"]["n_rx"], s, sl["delay"])
        mx, nv = max(mx, x), (nv + (noise // nest if nest else 0)) & 0xffffffff
    return mx, nv // sl["nvar_div"][0]


def with_measured(m, sl):
    """the slot with the measured max_ch / nvar in the true ones' place (two layers: what the receivers are fed on the device)"""
    if sl["case"]["n_layers"] == 1:
        return sl
    mx, nv = measured_host(m, sl)
    return dict(sl, max_ch=mx, nvar=nv)


def variants(m, sl):
    """name -> (gsegs, first): the descriptors a receiver that does not follow the rule of dmrs_symbol = 255 would use"""
    a, N, dmrs = sl["alloc"], sl["case"]["N"], sl["dmrs"]
    out = {"every symbol on the first DMRS symbol": m.pusch_grid_segments([dict(a, dmrs_symbol=dmrs[0])]),
           "every symbol on the last DMRS symbol": m.pusch_grid_segments([dict(a, dmrs_symbol=dmrs[-1])])}
    late = []
    for s in sl["gsegs"]:                                               # :1408 behind :1414: the DMRS symbol itself reads the span before
        sym = (s["rx_off"] - a["rx_slot_off"]) // N
        i = span_of(dmrs, sym)
        late.append(dict(s, ch_off=a["ch_off"] + dmrs[i - 1] * N) if sym == dmrs[i] and i > 0 else s)
    out["the spans one symbol late"] = (late, sl["first"])
    return out


def time_average_host(m, sl, ch):
    """chest_time = 1 on the CPU forms: (the averaged copy of ch, gsegs, first with the explicit first DMRS symbol, the avg descriptor)"""
    c = sl["case"]
    asegs, first_dmrs = m.pusch_chest_avg_segments([sl["alloc"]])
    out = ch.copy()
    for q in range(c["n_layers"] * c["n_rx"]):
        m.pusch_chest_time_avg_host(out, dict(asegs[0], ch_off=[o + q * sl["ch_stride"] for o in asegs[0]["ch_off"]]))
    gsegs, first = m.pusch_grid_segments([dict(sl["alloc"], dmrs_symbol=first_dmrs[0])])
    return out, gsegs, first, asegs[0]
