"""A float64 PUSCH slot on the OFDM grid with a frequency-selective channel, and the receive chain that must invert it: DMRS
channel estimation, channel level, compensation (one layer) or the two-layer MMSE receiver (below 64QAM: the max-log ML
receiver), de-mapping and decoding.  The model
knows nothing of csrc/ but what a transmitter has too: the layer planes of dlsch_encode_symbols_host and the conjugated pilots of
pusch_dmrs_host (the pilot on the air is their conjugate).  test_ul_slot_host.py runs the chain on the CPU forms, test_gpu_ul_slot.py
on the GPU, both on the slots of CASES.

The channel of layer l to antenna a at subcarrier k, counted from the allocation's first RE and continuous across the grid's wrap
(subcarriers N - 1 and 0 are neighbours):

    h[l, a](k) = g[l, a] exp(-2 pi i k tau[a] / N) + e[l, a] exp(-2 pi i k tau2 / N)

a main tap tau[a] whole samples late (negative: early) and a weak second tap that keeps the channel from being exactly flat once
the main tap's delay is taken out.  Data RE: y[a] = sum_l h[l, a](k) x[l] / 23170 + n.  DMRS RE: every transmitted port is on the
air in the same symbol, y[a] = sum_l h[l, a](k) conj(p_l) / (23170 sqrt 2) + n with p_l the port's conjugated pilot (w_f included)
on the port's comb: |p| = 23170 sqrt 2, so p y is 23170 sqrt 2 h, which two shift-16 products added or shift-15 products averaged
bring to h.  The noise n has the same sigma per component on both kinds of RE.

est_delay.  The delay tables hold row get_delay_idx(d) = clamp(20 + d, 0, 40) with entry k = round(256 exp(+2 pi i k d / N))
(nr_chest.h, nr_common.c:906-928).  TYPE1_INTERP multiplies the LS value of the pilot at RE 2 pc by entry 2 pc of row idx(d)
(nr_ul_channel_estimation.c:209-210), filters, and multiplies RE k by entry k of row idx(-d) (:239-245); TYPE2_INTERP multiplies RE
r of a 6-RE block by entry r of row idx(-d).  The forward rotation exp(+2 pi i k d / N) cancels the main tap's exp(-2 pi i k tau /
N) when d = tau, and the backward rotation then puts exp(-2 pi i k tau / N) back: est_delay is tau[a] itself, in samples of the
N-point grid, positive for a late tap, at most 20 in size, one value per (descriptor, antenna) at delay_off + a.  The two
averaging modes take no delay at all (the reference's NO_INTERP build has no table in it): est_delay is passed and ignored there.

The second layer.  Layer l, antenna a of ul_ch lies at (l n_rx + a) ch_stride, the plane order channel_level_grid_mmse and
mmse_2layers_grid read.  The estimator reaches it through a second descriptor set: pusch_chest_segments on the same allocation
with cfg.port = the layer's port, ch_off moved by l n_rx ch_stride and delay_off continued behind layer 0's (chest_descriptors).
"""
import numpy as np

import oracle_lib as O
import rx_chest_np as chest_ref
from layer_np import symbols_np
from qam_np import demap_np
from rx_front_np import compensate_np, level_np
from rx_ml_np import level_ml_np, llr_np, ml_np
from rx_mmse_np import level_mmse_np, mmse_np, records_np
from test_scrambling_host import c_init_of
from test_tb_scrambled_emul import unscramble

T1I, T2I, T1A, T2A = 0, 1, 2, 3
FULL, DMRS1, DMRS2 = 0, 1, 2
FILL = -4321                            # what ul_ch holds where nothing was estimated
GRID_FILL = 1234                        # and the grid where nothing was received
MAX_ITER = 8
SIGMA_1L = 75.0                         # e2e_slot of test_gpu_rx_chest.py: 0.05 * 1500 per component
SIGMA_2L = 3.0                          # E2E_SIGMA of test_rx_mmse_host.py
GAIN_2L = (400.0, 480.0)                # E2E_GAIN of test_rx_mmse_host.py


def _case(name, mode, ports, n_rx, Qm, N, tau, gain, e_rel, tau2, rate, seed, rb=10, cdm=1, BG=1, delay_factor=3.0, corr=0.0, survives=()):
    return dict(name=name, mode=mode, ports=ports, n_layers=len(ports), n_rx=n_rx, Qm=Qm, N=N, tau=tau, gain=gain, e_rel=e_rel, tau2=tau2,
                rate=rate, seed=seed, rb=rb, cdm=cdm, BG=BG, delay_checks=not ports[0] & 2, delay_factor=delay_factor,
                sigma=SIGMA_1L if len(ports) == 1 else SIGMA_2L, corr=corr, survives=survives)


def is_ml(case):
    """two layers below 64QAM go through the max-log ML receiver, which writes LLRs, not symbol records"""
    return case["n_layers"] == 2 and case["Qm"] < 6


# One layer: every estimator mode, port 0 (w_f constant), port 1 (w_f alternates) and port 2 (type 1, delta = 1; two CDM groups without
# data, so the DMRS symbol carries no data), n_rx 1, 2 and 4, Qm 4, 6 and 8.  Two layers: ports 0 and 1 on the air together, every
# mode, Qm 6 and 8, n_rx 2 and 4; the gain structure of mmse_e2e_case.  The delays are as large as the bounds of
# test_ul_slot_host.py allow each mode: the interpolating modes take the main tap's delay out, the averaging ones and the
# separation of two ports on one comb do not.  The code rates are high enough that an estimate a few REs off no longer decodes.
# delay_factor: by how much a wrong est_delay must miss the bound (test_ul_slot_host.py says why "2L-T1I" cannot reach 3).
# The last two go through the ML receiver (two layers, QPSK and 16QAM) with the layers' columns at correlation 0.6.  survives: the
# perturbations after which the block decodes all the same -- QPSK at 40 dB takes a negated delay's 25 degrees.
CASES = [
    _case("1L-T1I-p0", T1I, (0,), 2, 6, 256, (6, -5), (2200.0, 2600.0), 0.010, 9, 0.80, 11),
    _case("1L-T2I-p1", T2I, (1,), 4, 8, 512, (8, -7, 6, -8), (2200.0, 2600.0), 0.010, 11, 0.80, 12),
    _case("1L-T1A-p1", T1A, (1,), 1, 4, 512, (1,), (2200.0, 2600.0), 0.010, 3, 0.80, 13),
    _case("1L-T2A-p0", T2A, (0,), 2, 4, 512, (1, -1), (2000.0, 2200.0), 0.005, 3, 0.80, 14),
    _case("1L-T1I-p2", T1I, (2,), 2, 6, 256, (2, -1), (2200.0, 2600.0), 0.010, 6, 0.80, 15, cdm=2),
    _case("2L-T1I", T1I, (0, 1), 4, 8, 512, (7, -6, 5, -7), GAIN_2L, 0.007, 10, 0.60, 21, delay_factor=2.0),
    _case("2L-T2I", T2I, (0, 1), 2, 6, 512, (5, -4), GAIN_2L, 0.010, 9, 0.75, 22),
    _case("2L-T1A", T1A, (0, 1), 4, 6, 512, (1, -1, 1, -1), GAIN_2L, 0.010, 3, 0.75, 23),
    _case("2L-T2A", T2A, (0, 1), 2, 6, 512, (1, -1), GAIN_2L, 0.010, 3, 0.75, 24),
    # through the ML receiver, the layers' columns at correlation 0.6 (build_slot): 16QAM on four antennas, QPSK on two
    _case("2L-T1I-ml16", T1I, (0, 1), 4, 4, 512, (7, -6, 5, -7), GAIN_2L, 0.007, 10, 0.88, 31, delay_factor=2.0, corr=0.6),
    _case("2L-T1I-ml4", T1I, (0, 1), 2, 2, 512, (7, -6), GAIN_2L, 0.007, 10, 0.92, 32, delay_factor=2.0, corr=0.6, survives=("est_delay negated",)),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}


def _c16(z):
    return np.clip(np.rint(np.stack([z.real, z.imag], -1)), -32768, 32767).astype(np.int16)


def chest_descriptors(m, alloc, cfg, ports, n_rx, ch_stride):
    """One descriptor set per layer from pusch_chest_segments on the same allocation: cfg.port = the layer's port, ch_off moved by
    l n_rx ch_stride, delay_off continued behind the sets before it.  Returns the flat list, layer-major."""
    out = []
    for l, port in enumerate(ports):
        mine = m.pusch_chest_segments([alloc], [dict(cfg, port=port)], n_rx)
        out += [dict(c, ch_off=c["ch_off"] + l * n_rx * ch_stride, delay_off=c["delay_off"] + len(out) * n_rx) for c in mine]
    return out


def dmrs_res(mode, port, n_pil):
    """The REs, counted from the allocation's first, that carry the port's pilots 0 .. n_pil - 1 (38.211 6.4.1.1.3 for the ports used
    here: type 1 ports 0..3, k = 4 n + 2 k' + delta; type 2 ports 0 and 1, k = 6 n + k')"""
    k = np.arange(n_pil)
    if mode & 1:
        assert port in (0, 1)
        return 6 * (k // 2) + k % 2
    assert port in (0, 1, 2, 3)
    return 2 * k + ((port >> 1) & 1)


def channel_of(c, rng):
    """The case's channel on its allocation, drawn from rng: (g, e, h complex128 [n_layers, n_rx, 12 rb], h16, max_ch)"""
    N, rb, L, n_rx = c["N"], c["rb"], c["n_layers"], c["n_rx"]
    tau = np.array(c["tau"], np.float64)
    assert len(tau) == n_rx and np.abs(tau).max() <= 20 and (n_rx == 1 or (tau.min() < 0 < tau.max() and len(set(c["tau"])) > 1))
    gm, ph = rng.uniform(*c["gain"], n_rx), rng.uniform(0, 2 * np.pi, n_rx)
    col = gm * np.exp(1j * ph)
    if L == 1:
        g = col[None]
    else:                                                              # mmse_e2e_case: layer 1 is layer 0 turned and sign-alternated
        o = col * np.exp(1j * rng.uniform(0, 2 * np.pi)) * (-1.0) ** np.arange(n_rx)
        if c["corr"]:
            # ... plus corr times layer 0's column a quarter turn from it: every path keeps its gain, |c j + sqrt(1 - c^2)| = 1, and
            # the columns' correlation is corr but for the spread of the gains
            o = 1j * c["corr"] * o / (-1.0) ** np.arange(n_rx) + np.sqrt(1.0 - c["corr"] ** 2) * o
            assert abs(abs(np.vdot(col, o)) / (np.linalg.norm(col) * np.linalg.norm(o)) - c["corr"]) < 0.03
        g = np.stack([col, o])
    e = c["e_rel"] * np.abs(g) * np.exp(1j * rng.uniform(0, 2 * np.pi, g.shape))
    k = np.arange(12 * rb)
    h = (g[..., None] * np.exp(-2j * np.pi * k * tau[None, :, None] / N) + e[..., None] * np.exp(-2j * np.pi * k * c["tau2"] / N))
    h16 = _c16(h)
    if L == 2:                                                         # the band DESIGN 4.11.1 names: log2_approx of the level stays 18
        assert (np.abs(h) ** 2 >= 2 ** 17).all() and (np.abs(h) ** 2 < 2 ** 18).all()
    max_ch = int(np.abs(h16.astype(np.int32)).max())
    assert L == 1 or max_ch < 2048                                     # shift_ch_ext = 0 in the MMSE level
    return g, e, h, h16, max_ch


def span_of(dmrs, symbol):
    """which DMRS symbol (index into dmrs) serves `symbol`: the latest at or before it, the first in front of it"""
    return max(sum(d <= symbol for d in dmrs) - 1, 0)


def build_slot(m, case, dmrs=None, f_span=None, rng_seed=None):
    """The transport block, its descriptors and the slot of one case.  Returns a dict: tb, scr, pay, alloc, gsegs, first, csegs (every
    layer's), delay (int32 per (descriptor, antenna): tau[a]), rx (int16 [n_rx, rx_stride, 2]), rx_stride, ch_stride, h (complex128
    [n_layers, n_rx, 12 rb]: the true channel on the allocation), h16 (its rounding to int16 [.., 2]), g, e, max_ch (the largest
    component of h16) and nvar = 2 sigma^2.
    By default one DMRS symbol (2 or 3 by the seed), named in alloc.dmrs_symbol.  ul_slot_tv_np.py passes dmrs = several DMRS symbols
    (alloc.dmrs_symbol = 255; csegs layer-major, within a layer in symbol order) and f_span = a complex factor on the channel per
    DMRS symbol, which holds from that symbol to the next (span_of); h stays the channel without it, max_ch is taken with it."""
    from test_gpu_tb_chain import valid_tbs
    c = case
    rng = np.random.default_rng(9000 + c["seed"] if rng_seed is None else rng_seed)
    N, rb, L, n_rx, Qm, typ = c["N"], c["rb"], c["n_layers"], c["n_rx"], c["Qm"], c["mode"] & 1
    n_rb = N // 12 - 1 - (N // 12 - 1) % 2                              # the carrier's width: the wrap lies between two PRBs
    rb_start = n_rb // 2 - rb // 2                                      # half of the allocation on either side of the wrap
    follow = dmrs is not None
    dmrs = tuple(dmrs) if follow else (2 + (c["seed"] & 1),)
    n_dm = len(dmrs)
    f_span = np.ones(n_dm, np.complex128) if f_span is None else np.asarray(f_span, np.complex128)
    S = (14 - n_dm) * 12 * rb + n_dm * ((8 if typ else 6) * rb if c["cdm"] == 1 else 0)  # data REs per layer
    G = Qm * L * S
    tb = dict(A=valid_tbs(int(G * c["rate"]), c["BG"]), G=G, BG=c["BG"], Qm=Qm, Nl=L, rv=0, tbslbrm=0)
    scr = (int(rng.integers(0, 0x10000)), 0, int(rng.integers(0, 1024)))
    pay = rng.integers(0, 256, tb["A"] // 8, dtype=np.uint8)
    rx_stride, ch_stride = 14 * N + 9, 14 * N + 64
    alloc = dict(tb=0, Qm=Qm, dmrs_config_type=typ, num_dmrs_cdm_grps_no_data=c["cdm"], dmrs_symbol=255 if follow else dmrs[0], fft_size=N,
                 first_carrier_offset=N - 6 * n_rb, bwp_start=0, rb_start=rb_start, rb_size=rb, start_symbol=0, nr_of_symbols=14,
                 ul_dmrs_symb_pos=sum(1 << d for d in dmrs), plane=G // Qm, rx_slot_off=5, ch_off=7, rec_off=0)
    cfg = dict(slot=int(rng.integers(0, 20)), scid=c["seed"] & 1, dmrs_scrambling_id=int(rng.integers(0, 65536)), port=c["ports"][0],
               chest_freq=c["mode"] >> 1)
    gsegs, first = m.pusch_grid_segments([alloc])
    csegs = chest_descriptors(m, alloc, cfg, c["ports"], n_rx, ch_stride)
    assert len(csegs) == L * n_dm and all(s["mode"] == c["mode"] for s in csegs) and sum(s["nb_re"] for s in gsegs) == S
    assert [(s["rx_off"] - alloc["rx_slot_off"]) // N for s in csegs] == list(dmrs) * L
    k0 = csegs[0]["start_re"]
    assert k0 + 12 * rb > N and 24 <= N - k0 <= 12 * rb - 24, "a PRB pair lies on each side of the wrap"
    g, e, h, h16, max_ch = channel_of(c, rng)
    max_ch = int(np.abs(_c16(h[None] * f_span[:, None, None, None]).astype(np.int32)).max())
    assert L == 1 or (max_ch < 2048 and (np.abs(h * np.abs(f_span).max()) ** 2 < 2 ** 18).all())
    # the slot
    tx = symbols_np(O.dlsch_encode(tb, pay), scr, Qm, L)              # = dlsch_encode_symbols_host, which needs a GPU (the GPU test checks)
    assert tx.shape == (L, S, 2)
    x = (tx[..., 0].astype(np.float64) + 1j * tx[..., 1]) / 23170.0
    rx = np.full((n_rx, rx_stride, 2), GRID_FILL, np.int16)

    def put(at, v):
        v = v + c["sigma"] * (rng.standard_normal(v.shape) + 1j * rng.standard_normal(v.shape))
        rx[:, at] = _c16(v)
    for s in gsegs:
        f = f_span[span_of(dmrs, (s["rx_off"] - alloc["rx_slot_off"]) // N)]
        j = np.arange(s["nb_re"])
        p_j = {FULL: j, DMRS1: 2 * j + 1, DMRS2: 6 * (j // 4) + 2 + j % 4}[s["pattern"]]
        put(s["rx_off"] + (s["start_re"] + p_j) % N, f * np.einsum("lar,lr->ar", h[:, :, p_j], x[:, s["sym_off"]:s["sym_off"] + s["nb_re"]]))
    n_pil = (4 if typ else 6) * rb
    for i in range(n_dm):                                              # each DMRS symbol on the air with its span's factor
        dm = np.zeros((n_rx, 12 * rb), np.complex128)
        used = np.zeros(12 * rb, bool)
        for l in range(L):
            cs = csegs[l * n_dm + i]
            p = m.pusch_dmrs_host(cs["c_init"], cs["dmrs_offset"], n_pil, cs["port"], typ).astype(np.float64)
            re = dmrs_res(c["mode"], cs["port"], n_pil)
            dm[:, re] += f_span[i] * h[l][:, re] * (p[:, 0] - 1j * p[:, 1])[None, :] / (23170.0 * np.sqrt(2.0))
            used[re] = True
        re = np.flatnonzero(used)
        put(csegs[i]["rx_off"] + (k0 + re) % N, dm[:, re])
    delay = np.array([c["tau"][a] for _ in csegs for a in range(n_rx)], np.int32)
    return dict(case=c, tb=tb, scr=scr, pay=pay, alloc=alloc, gsegs=gsegs, first=first, csegs=csegs, delay=delay, rx=rx, rx_stride=rx_stride,
                ch_stride=ch_stride, tx=tx, h=h, h16=h16, g=g, e=e, max_ch=max_ch, nvar=int(round(2 * c["sigma"] ** 2)), dmrs=dmrs, f_span=f_span)


_SLOTS = {}


def slot_of(m, name):
    """The case's slot, built once per session and shared; nobody writes to it."""
    if name not in _SLOTS:
        _SLOTS[name] = build_slot(m, CASE_BY_NAME[name])
        for v in _SLOTS[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _SLOTS[name]


# ---- estimation ----------------------------------------------------------------------------------------------------------
def estimate_host(m, sl, delay=None, csegs=None):
    """ul_ch int16 [n_layers n_rx ch_stride, 2] out of pusch_chest_host per (descriptor, antenna), FILL elsewhere"""
    c = sl["case"]
    delay, csegs = sl["delay"] if delay is None else delay, sl["csegs"] if csegs is None else csegs
    ch = np.full((c["n_layers"] * c["n_rx"] * sl["ch_stride"], 2), FILL, np.int16)
    rx = np.ascontiguousarray(sl["rx"].reshape(-1, 2))
    for s in csegs:
        for a in range(c["n_rx"]):
            m.pusch_chest_host(rx, dict(s, rx_off=s["rx_off"] + a * sl["rx_stride"], ch_off=s["ch_off"] + a * sl["ch_stride"]),
                               int(delay[s["delay_off"] + a]), ch)
    return ch


def estimate_ref(sl):
    """the same array out of the literal restatement of the reference (rx_chest_np.py), one DMRS symbol of one antenna at a time"""
    c, N = sl["case"], sl["case"]["N"]
    ch = np.full((c["n_layers"] * c["n_rx"] * sl["ch_stride"], 2), FILL, np.int16)
    re_offset = 12 * (sl["alloc"]["bwp_start"] + sl["alloc"]["rb_start"])
    for s in sl["csegs"]:
        assert s["dmrs_offset"] == re_offset // (3 if s["mode"] & 1 else 2)
        for a in range(c["n_rx"]):
            sym = [(int(r), int(i)) for r, i in sl["rx"][a, s["rx_off"]:s["rx_off"] + N]] + [(0, 0)]
            out = chest_ref.pusch_channel_estimation(sym, 0, N, s["start_re"], s["rb_size"], s["port"], s["mode"] & 1, s["mode"] >> 1, s["c_init"],
                                                     re_offset, int(sl["delay"][s["delay_off"] + a]), literal_type2_avg=False)
            at = s["ch_off"] + a * sl["ch_stride"]
            ch[at:at + 12 * s["rb_size"]] = np.array(out[:12 * s["rb_size"]], np.int64).astype(np.int16)
    return ch


def planes_of(sl, ch):
    """the estimates on the allocation: a view int16 [n_layers, n_rx, 12 rb, 2] of ul_ch"""
    c = sl["case"]
    at = sl["csegs"][0]["ch_off"]
    return ch.reshape(c["n_layers"], c["n_rx"], sl["ch_stride"], 2)[:, :, at:at + 12 * c["rb"]]


def edge_mask(sl):
    """the first and last two 4-RE groups of the allocation, where the interpolation filters are one-sided"""
    n = 12 * sl["case"]["rb"]
    mask = np.zeros(n, bool)
    mask[:8] = mask[n - 8:] = True
    return mask


def est_error(sl, ch):
    """(interior, edge): the largest |est - h| per component over the REs of each kind, every layer and antenna"""
    d = np.abs(planes_of(sl, ch).astype(np.float64) - np.stack([sl["h"].real, sl["h"].imag], -1)).max(axis=(0, 1, 3))
    edge = edge_mask(sl)
    return float(d[~edge].max()), float(d[edge].max())


# ---- the receivers behind the estimates ----------------------------------------------------------------------------------
def _extract(sl, ch, s):
    """rx int16 [n_rx, nb_re, 2] and ch int16 [n_layers n_rx, nb_re, 2] of a grid segment (the closed form of nr_rx_grid.h)"""
    c = sl["case"]
    j = np.arange(s["nb_re"])
    p_j = {FULL: j, DMRS1: 2 * j + 1, DMRS2: 6 * (j // 4) + 2 + j % 4}[s["pattern"]]
    chp = ch.reshape(c["n_layers"] * c["n_rx"], sl["ch_stride"], 2)
    return (np.ascontiguousarray(sl["rx"][:, s["rx_off"] + (s["start_re"] + p_j) % c["N"]]), np.ascontiguousarray(chp[:, s["ch_off"] + p_j]))


def front_records(sl, ch, m=None):
    """(level shift, the block's symbol record int16 [G]) from ul_ch: level and compensation (one layer) or level_mmse and the
    two-layer MMSE receiver, segment by segment on extracted arrays.  m = the package's ldpc module: its CPU forms; m = None: the
    numpy restatements of the reference."""
    c, tb = sl["case"], sl["tb"]
    n_rx, Qm, plane = c["n_rx"], c["Qm"], tb["G"] // c["Qm"]
    rec = np.zeros(tb["G"], np.int16)
    f = sl["first"][0]
    chf = _extract(sl, ch, f)[1]
    if c["n_layers"] == 1:
        lv = int(m.ulsch_level_host(chf, n_rx, f["nb_re"], f["nb_re"])[0]) if m else int(level_np(chf)[0])
        for s in sl["gsegs"]:
            a, b = _extract(sl, ch, s)
            out = m.ulsch_compensate_host(a, b, n_rx, s["nb_re"], s["nb_re"], Qm, lv) if m else compensate_np(a, b, Qm, lv)
            rec.reshape(Qm // 2, plane, 2)[:, s["sym_off"]:s["sym_off"] + s["nb_re"]] = out
    elif is_ml(c):                                                     # the "record" is the block's LLRs
        if m:
            lv = int(m.ulsch_level_ml_host(chf, n_rx, f["nb_re"], f["nb_re"], sl["max_ch"])[0])
        else:
            lv = int(level_ml_np(chf.reshape(2, n_rx, f["nb_re"], 2), sl["max_ch"])[0])
        for s in sl["gsegs"]:
            a, b = _extract(sl, ch, s)
            out = m.ulsch_ml_2layers_host(a, b, n_rx, s["nb_re"], s["nb_re"], Qm, lv) if m else ml_np(a, b.reshape(2, n_rx, s["nb_re"], 2), Qm, lv)
            llr_np(rec, out, Qm, s["sym_off"])
    else:
        if m:
            lv = int(m.ulsch_level_mmse_host(chf, n_rx, f["nb_re"], f["nb_re"], sl["max_ch"])[0])
        else:
            lv = int(level_mmse_np(chf.reshape(2, n_rx, f["nb_re"], 2), sl["max_ch"])[0])
        for s in sl["gsegs"]:
            a, b = _extract(sl, ch, s)
            if m:
                out = m.ulsch_mmse_2layers_host(a, b, n_rx, s["nb_re"], s["nb_re"], Qm, lv, sl["nvar"])
            else:
                out = mmse_np(a, b.reshape(2, n_rx, s["nb_re"], 2), Qm, lv, sl["nvar"])
            records_np(rec, out, Qm, plane, s["sym_off"])
    return lv, rec


def decode_record(sl, rec):
    """(payload, ack, per-segment pass counts) of the record through demap_np (the ML receiver's LLRs: as they are), unscramble and
    the oracle's decoder"""
    tb, Qm = sl["tb"], sl["case"]["Qm"]
    pl = rec.reshape(Qm // 2, tb["G"] // Qm, 2)
    llr = unscramble(rec if is_ml(sl["case"]) else demap_np(pl[0], list(pl[1:]), Qm), c_init_of(*sl["scr"]), 0)
    s = O.segmentation(None, O.len_with_crc(1, tb["A"]), tb["BG"])
    harq = [np.zeros(66 * 384 + 16, np.int16) for _ in range(s["C"])]
    got, ack, iters, _ = O.ulsch_decode(tb, llr, harq, MAX_ITER)
    return got, ack, iters
