"""What test_gpu_callers.py issues and what it expects: device-mode calls as objects that are staged (inputs and canary-filled
outputs to the GPU), issued (nothing but the library's calls, on a stream given as an integer) and read back at different times,
by different threads.  Every expectation comes from the CPU forms and numpy restatements the other tests hold the kernels to
(pusch_chest_host, ulsch_extract_host + ulsch_level_host / ulsch_compensate_host, pdsch_precode_host, rx_mmse_np, symbols_np, the
oracle chain) and is computed when the call object is built: single-threaded, before any thread starts.

Variants.  The *_calls(m, K) builders return K calls of one entry point that may follow each other through one thread context
without a fault even if the library mixed their descriptor tables up: the tables have the same counts and address the same ranges
of same-sized arrays, and differ only in values that change what is computed -- c_init, port, est_delay, amp, the PMIs, the
block a grid descriptor belongs to (its shift and noise variance), rv, the scrambling identity, the data.  differs() says by how much
the expectations of two calls differ."""
import numpy as np

import oracle_lib as O
import ul_slot_np as U
from layer_np import symbols_np
from qam_np import demap_np
from test_gpu_slot_calls import CANARY, N_ANT, QM, slot_case
from test_gpu_tb_chain import valid_tbs
from test_gpu_tb_scr_oracle import rx_inputs, scr_bits
from test_scrambling_host import c_init_of
from test_tb_scrambled_emul import unscramble

CANARY8 = 0x5a
MAX_ITER = 8


class Call:
    """want: {name: expected numpy array}.  stage(stream) -> self: the device tensors, made on the current stream (before any delay
    is queued; stream = where the call will be issued, for the calls that must know early).  issue(stream): the library's calls
    and nothing else.  got(): {name: numpy array} of the outputs named in want."""

    def __init__(self, want, stage, issue):
        self.want, self._stage, self._issue, self.dev = want, stage, issue, None

    def stage(self, stream=None):
        self.dev = self._stage(stream)
        return self

    def issue(self, stream):
        self._issue(self.dev, stream)

    def got(self):
        return {k: self.dev[k].cpu().numpy().reshape(-1) for k in self.want}

    def mismatches(self, tag):
        """[] or one entry per output that differs from its expectation: (tag, name, first differing indices)"""
        out = []
        for k, v in self.got().items():
            w = self.want[k].reshape(-1)
            if v.shape != w.shape or not np.array_equal(v, w):
                out.append((tag, k, np.flatnonzero(v != w)[:6].tolist() if v.shape == w.shape else (v.shape, w.shape)))
        return out


BACKGROUND = dict(harq=0, coded=0x5a, pay=None)     # what an output holds where no call writes; every other output: CANARY


def differs(a, b):
    """the smallest fraction, over the outputs of two calls, of entries in which their expectations differ, among the entries that
    at least one of the two writes (single numbers -- ACK, pass count -- apart)"""
    out = []
    for k in a.want:
        x, y = a.want[k].reshape(-1), b.want[k].reshape(-1)
        if x.size > 4:
            bg = BACKGROUND.get(k, CANARY)
            written = np.ones(x.size, bool) if bg is None else (x != bg) | (y != bg)
            out.append(float(np.mean(x[written] != y[written])))
    return min(out)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()


def fill(n, v=CANARY, dt="int16"):
    import torch
    return torch.full((int(n),), v, dtype=getattr(torch, dt), device="cuda")


# ---- the oracle's decode of one transport block ------------------------------------------------------------------------------
def decode_want(m, tb, llr):
    """{pay, ack, itm, harq} of a first transmission as the device-mode decode calls leave them: the payload (zeros when the block
    is lost: compared only where the oracle ACKs, see decode_outputs), ACK, the largest pass count, the soft buffers row by row"""
    C_ = O.segmentation(None, O.len_with_crc(1, tb["A"]), tb["BG"])["C"]
    harq = [np.zeros(m.HARQ_STRIDE, np.int16) for _ in range(C_)]
    pay, ack, its, _ = O.ulsch_decode(dict(tb), llr, harq, MAX_ITER, 0, 0, vec=True)
    want = dict(ack=np.array([1 if ack else 0], np.uint8), itm=np.array([max(its)], np.int32), harq=np.concatenate(harq))
    if ack:
        want["pay"] = np.asarray(pay, np.uint8)[:tb["A"] // 8]
    return want


def decode_outputs(m, tb, want):
    """the device tensors a decode call writes, by the names of decode_want; _out is the whole payload array"""
    import torch
    po, _, ho, _ = m.tb_layout([tb])
    d = dict(harq=torch.zeros(int(ho[-1]), dtype=torch.int16, device="cuda"), _out=fill(int(po[-1]) + 16, 0, "uint8"),
             ack=fill(1, 7, "uint8"), itm=fill(1, -7, "int32"))
    if "pay" in want:
        d["pay"] = d["_out"][:tb["A"] // 8]
    return d


# ---- a DL slot: payload -> layer planes -> precoded transmit grid ---------------------------------------------------------------
_dl = {}


def dl_slot(m, N, rb, seed, var=0, n_tx=4):
    """One PDSCH allocation of rb PRBs over 14 symbols on an N-point grid, the first PRB at the grid's end so that the rest wraps
    round it (first_carrier_offset = N - 12), two layers of 16QAM on n_tx antennas through one PMI per PRB.  The layer planes start
    at int16 6 of their array (byte 12), the grid at c16 1 of each antenna.  seed: payload, scrambling identity, matrices.  var: a
    variant in the sense of the module docstring -- another amp, DMRS scrambling identity, scid and PMI list.  A dict: tb, pay, scr,
    lay (int16, CANARY around the planes), segs, prgs, pmis, table, ts (antenna stride), tx (int16 [n_tx ts, 2], CANARY where
    nothing is written)."""
    key = (N, rb, seed, var, n_tx)
    if key in _dl:
        return _dl[key]
    rng = np.random.default_rng(7000 + seed)
    Nl, Qm, S = 2, 4, (13 * 12 + 6) * rb
    G = Qm * Nl * S
    tb = dict(A=valid_tbs(G // 2, 2 if G // 2 <= 3824 else 1), G=G, BG=2 if G // 2 <= 3824 else 1, Qm=Qm, Nl=Nl, rv=0, tbslbrm=0)
    scr = (int(rng.integers(0, 0x10000)), int(rng.integers(0, 2)), int(rng.integers(0, 1024)))
    pay = rng.integers(0, 256, tb["A"] // 8, dtype=np.uint8)
    planes = symbols_np(O.dlsch_encode(tb, pay), scr, Qm, Nl)
    assert planes.shape == (Nl, S, 2)
    lay = np.full(6 + 2 * Nl * S + 8, CANARY, np.int16)
    lay[6:6 + 2 * Nl * S] = planes.reshape(-1)
    alloc = dict(Nl=Nl, plane=S, dmrs_config_type=0, num_dmrs_cdm_grps_no_data=1, dmrs_ports=0b11, scid=(seed + var) & 1,
                 dl_dmrs_scrambling_id=99 + 37 * var, slot=4, si_rnti=0, amp=512 + 111 * var, fft_size=N, first_carrier_offset=N - 12, bwp_start=0,
                 rb_start=0, rb_size=rb, start_symbol=0, nr_of_symbols=14, dl_dmrs_symb_pos=1 << 2, tx_slot_off=1, lay_off=6)
    table = [dict(pm_idx=t + 1, numLayers=Nl, num_ant_ports=n_tx, weights=rng.integers(-23170, 23171, (Nl, n_tx, 2)).astype(np.int16)) for t in range(3)]
    pmis = [(1, 0, 3, 2, 2, 1, 3)[(q + var) % 7] for q in range(rb)]    # PMI 0: the unit matrix, antenna a carries layer a
    segs, prgs = m.pdsch_precode_segments([alloc], [dict(prg_size=1, pmi_off=0, pmi_count=rb)], len(pmis))
    assert len(segs) == 14 and segs[0]["start_re"] == N - 12 and segs[0]["start_re"] + 12 * rb > N
    ts = 14 * N + 1 + 4
    tx = np.full((n_tx * ts, 2), CANARY, np.int16)
    for s, g in zip(segs, prgs):
        for a in range(n_tx):
            m.pdsch_precode_host(lay, dict(s, tx_off=s["tx_off"] + a * ts), g, pmis, table, n_tx, a, tx)
    assert (tx[0] == CANARY).all() and (tx[-4:] == CANARY).all() and (tx != CANARY).any()
    _dl[key] = dict(N=N, rb=rb, S=S, n_tx=n_tx, tb=tb, pay=pay, scr=scr, lay=lay, segs=segs, prgs=prgs, pmis=pmis, table=table, ts=ts, tx=tx)
    return _dl[key]


def map_call(m, d):
    """pdsch_resource_mapping_precoded on the slot's layer planes"""
    return Call(dict(tx=d["tx"]), lambda s: dict(lay=dev(d["lay"]), tx=fill(d["tx"].size)),
                lambda t, s: m.pdsch_resource_mapping_precoded(t["lay"], t["tx"], d["ts"], d["n_tx"], d["segs"], d["prgs"], d["pmis"], d["table"], stream=s))


def map_host(m, d):
    tx = np.full(d["tx"].size, CANARY, np.int16)
    m.pdsch_resource_mapping_precoded(d["lay"], tx, d["ts"], d["n_tx"], d["segs"], d["prgs"], d["pmis"], d["table"])
    return dict(tx=tx)


def payload_dev(m, tb, pay):
    po = m.tb_layout([tb])[0]
    h = np.zeros(int(po[-1]) + 16, np.uint8)
    h[:pay.size] = pay
    return dev(h)


def encsym_call(m, d):
    """dlsch_encode_symbols_device into the slot's layer array"""
    return Call(dict(lay=d["lay"]), lambda s: dict(pay=payload_dev(m, d["tb"], d["pay"]), lay=fill(d["lay"].size)),
                lambda t, s: m.dlsch_encode_symbols_device([d["tb"]], t["pay"], t["lay"], [d["scr"]], stream=s, coded_off=[12]))


def dl_chain_call(m, d):
    """payload bytes -> layer planes -> precoded grid: two calls on one stream"""
    def issue(t, s):
        m.dlsch_encode_symbols_device([d["tb"]], t["pay"], t["lay"], [d["scr"]], stream=s, coded_off=[12])
        m.pdsch_resource_mapping_precoded(t["lay"], t["tx"], d["ts"], d["n_tx"], d["segs"], d["prgs"], d["pmis"], d["table"], stream=s)
    return Call(dict(lay=d["lay"], tx=d["tx"]), lambda s: dict(pay=payload_dev(m, d["tb"], d["pay"]), lay=fill(d["lay"].size), tx=fill(d["tx"].size)), issue)


def map_calls(m, K, N=256, rb=3):
    return [map_call(m, dl_slot(m, N, rb, 40, var=k)) for k in range(K)]


def encsym_calls(m, K, N=256, rb=3):
    return [encsym_call(m, dl_slot(m, N, rb, 50 + k)) for k in range(K)]


# ---- one layer: the slot of test_gpu_slot_calls.py through estimation, level, compensation and decoding -----------------------------
def est_calls(m, K, N=256, rb=3):
    """pusch_channel_estimation on slot_case's grid: variant k has its own c_init, port (0 and 1: one comb) and est_delay"""
    c = slot_case(m, N, rb)
    calls = []
    for k in range(K):
        segs = [dict(s, c_init=(s["c_init"] + 7919 * k) & 0x7fffffff, port=k & 1) for s in c["csegs"]]
        delay = (c["delay"] + np.array([k, -k])).astype(np.int32)
        ch = np.full(c["ch"].shape, CANARY, np.int16)
        for s in segs:
            for a in range(N_ANT):
                m.pusch_chest_host(c["rx"], dict(s, rx_off=s["rx_off"] + a * c["rs"], ch_off=s["ch_off"] + a * c["cs"]), int(delay[s["delay_off"] + a]), ch)
        calls.append(Call(dict(ch=ch), lambda s, delay=delay: dict(rx=dev(c["rx"]), delay=dev(delay), ch=fill(c["ch"].size)),
                          lambda t, s, segs=segs: m.pusch_channel_estimation(t["rx"], c["rs"], t["ch"], c["cs"], N_ANT, segs, t["delay"], stream=s)))
    return calls


def ul1_chain_call(m, N, rb):
    """slot_case(m, N, rb): estimation -> level -> compensation -> decode_symbols on one stream, every intermediate an output.  The
    grid is random, so the block is lost: ACK 0, the pass count of a decoder that never converges, and the soft buffers are what
    the oracle makes of the record."""
    c = slot_case(m, N, rb)
    G = QM * c["S"]
    tb = dict(A=valid_tbs(G // 2, 2 if G // 2 <= 3824 else 1), G=G, BG=2 if G // 2 <= 3824 else 1, Qm=QM, Nl=1, rv=0, tbslbrm=0, round=0, llrLen=0)
    scr = (1000 + rb, 0, 17 * rb)
    pl = c["rec"][2:2 + G].reshape(QM // 2, G // QM, 2)
    dec = decode_want(m, tb, unscramble(demap_np(pl[0], list(pl[1:]), QM), c_init_of(*scr), 0))
    want = dict(dec, ch=c["ch"], lv=np.array([c["lv"], -7], np.int32), rec=c["rec"])

    def stage(s):
        return dict(decode_outputs(m, tb, dec), rx=dev(c["rx"]), delay=dev(c["delay"]), ch=fill(c["ch"].size), lv=fill(2, -7, "int32"),
                    rec=fill(c["rec"].size))

    def issue(t, s):
        m.pusch_channel_estimation(t["rx"], c["rs"], t["ch"], c["cs"], N_ANT, c["csegs"], t["delay"], stream=s)
        m.ulsch_channel_level_grid(t["ch"], N_ANT, c["cs"], c["first"], out=t["lv"], stream=s)
        m.ulsch_channel_compensation_grid(t["rx"], t["ch"], N_ANT, c["rs"], c["cs"], c["gsegs"], t["lv"], t["rec"], stream=s)
        m.ulsch_decode_symbols_device([dict(tb)], t["rec"][2:], t["harq"], t["_out"], t["ack"], t["itm"], [scr], stream=s)
    return Call(want, stage, issue)


# ---- two layers: a slot of ul_slot_np.py through estimation, MMSE level, the MMSE receiver and decoding ----------------------------
_ul2 = {}


def ul2_slot(m, N, rb, seed, mode=U.T2I):
    """a two-layer slot of ul_slot_np.py (ports 0 and 1, two antennas, 64QAM) at another grid size and width, with what the CPU side
    makes of it: ch (estimate_host), lv and rec (the numpy MMSE receiver on those estimates), dec (the oracle on that record)"""
    key = (N, rb, seed, mode)
    if key not in _ul2:
        sl = U.build_slot(m, U._case("2L-%d-%d" % (N, rb), mode, (0, 1), 2, 6, N, (5, -4), U.GAIN_2L, 0.010, 9, 0.60, seed, rb=rb))
        ch = U.estimate_host(m, sl)
        lv, rec = U.front_records(sl, ch, None)
        pl = rec.reshape(3, sl["tb"]["G"] // 6, 2)
        dec = decode_want(m, sl["tb"], unscramble(demap_np(pl[0], list(pl[1:]), 6), c_init_of(*sl["scr"]), 0))
        _ul2[key] = dict(sl, ch=ch, lv=lv, rec=rec, dec=dec)
    return _ul2[key]


def mmse_want(sl, segs=None):
    rec = sl["rec"] if segs is None else U.front_records(dict(sl, gsegs=segs), sl["ch"], None)[1]
    return np.concatenate([rec, np.full(16, CANARY, np.int16)])


def mmse_inputs(sl):
    import torch
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device="cuda")
    return dict(rx=dev(sl["rx"]), chin=dev(sl["ch"]), lvin=i32(sl["lv"]), nv=i32(sl["nvar"]), mc=i32(sl["max_ch"]))


def level_mmse_call(m, sl):
    n_rx = sl["case"]["n_rx"]
    return Call(dict(lv=np.array([sl["lv"], -7], np.int32)), lambda s: dict(mmse_inputs(sl), lv=fill(2, -7, "int32")),
                lambda t, s: m.ulsch_channel_level_grid_mmse(t["chin"], n_rx, sl["ch_stride"], sl["first"], t["mc"], out=t["lv"], stream=s))


def mmse_call(m, sl, segs=None):
    """ulsch_mmse_2layers_grid on the slot's grid and the CPU side's estimates; segs: other grid descriptors than the slot's"""
    n_rx, segs = sl["case"]["n_rx"], sl["gsegs"] if segs is None else segs
    want = mmse_want(sl, segs)
    return Call(dict(rec=want), lambda s: dict(mmse_inputs(sl), rec=fill(want.size)),
                lambda t, s: m.ulsch_mmse_2layers_grid(t["rx"], t["chin"], n_rx, sl["rx_stride"], sl["ch_stride"], segs, t["lvin"], t["nv"], t["rec"], stream=s))


def level_mmse_host(m, sl):
    """ulsch_channel_level_grid_mmse in HOST mode on the CPU side's estimates, in the shape of level_mmse_call's output"""
    lv = m.ulsch_channel_level_grid_mmse(np.ascontiguousarray(sl["ch"]).reshape(-1), sl["case"]["n_rx"], sl["ch_stride"], sl["first"],
                                         np.array([sl["max_ch"]], np.int32))
    return dict(lv=np.array([lv[0], -7], np.int32))


def mmse_host(m, sl):
    """ulsch_mmse_2layers_grid in HOST mode on the CPU side's estimates and level"""
    rec = np.full(sl["rec"].size + 16, CANARY, np.int16)
    m.ulsch_mmse_2layers_grid(np.ascontiguousarray(sl["rx"]).reshape(-1), np.ascontiguousarray(sl["ch"]).reshape(-1), sl["case"]["n_rx"], sl["rx_stride"],
                              sl["ch_stride"], sl["gsegs"], np.array([sl["lv"]], np.int32), np.array([sl["nvar"]], np.int32), rec)
    return dict(rec=rec)


def mmse_calls(m, K):
    """ulsch_mmse_2layers_grid with shift and nvar arrays of K entries: variant k's descriptors name block k, whose shift is k
    above the slot's level and whose noise variance is its own; grid, estimates and record array are the same"""
    import torch
    from rx_mmse_np import mmse_np, records_np
    sl = ul2_slot(m, 256, 4, 31)
    n_rx, G = sl["case"]["n_rx"], sl["tb"]["G"]
    shifts, nvars = [sl["lv"] + k for k in range(K)], [sl["nvar"] * (1 + 97 * k) for k in range(K)]
    calls = []
    for k in range(K):
        segs = [dict(s, tb=k) for s in sl["gsegs"]]
        rec = np.zeros(G, np.int16)
        for s in sl["gsegs"]:
            a, b = U._extract(sl, sl["ch"], s)
            records_np(rec, mmse_np(a, b.reshape(2, n_rx, s["nb_re"], 2), 6, shifts[k], nvars[k]), 6, G // 6, s["sym_off"])
        want = np.concatenate([rec, np.full(16, CANARY, np.int16)])
        calls.append(Call(dict(rec=want),
                          lambda s, n=want.size: dict(rx=dev(sl["rx"]), chin=dev(sl["ch"]), lvin=torch.tensor(shifts, dtype=torch.int32, device="cuda"),
                                                      nv=torch.tensor(nvars, dtype=torch.int32, device="cuda"), rec=fill(n)),
                          lambda t, s, segs=segs: m.ulsch_mmse_2layers_grid(t["rx"], t["chin"], n_rx, sl["rx_stride"], sl["ch_stride"], segs, t["lvin"], t["nv"],
                                                                            t["rec"], stream=s)))
    assert np.array_equal(calls[0].want["rec"], mmse_want(sl))
    return calls


def ul2_chain_call(m, sl):
    """estimation (both layers' descriptors) -> MMSE level -> MMSE receiver -> decode_symbols on one stream"""
    n_rx = sl["case"]["n_rx"]
    tb = dict(sl["tb"], round=0, llrLen=0)
    want = dict(sl["dec"], ch=sl["ch"], lv=np.array([sl["lv"], -7], np.int32), rec=mmse_want(sl))

    def stage(s):
        t = mmse_inputs(sl)
        return dict(decode_outputs(m, tb, sl["dec"]), rx=t["rx"], nv=t["nv"], mc=t["mc"], delay=dev(sl["delay"]), ch=fill(sl["ch"].size, U.FILL),
                    lv=fill(2, -7, "int32"), rec=fill(want["rec"].size))

    def issue(t, s):
        m.pusch_channel_estimation(t["rx"], sl["rx_stride"], t["ch"], sl["ch_stride"], n_rx, sl["csegs"], t["delay"], stream=s)
        m.ulsch_channel_level_grid_mmse(t["ch"], n_rx, sl["ch_stride"], sl["first"], t["mc"], out=t["lv"], stream=s)
        m.ulsch_mmse_2layers_grid(t["rx"], t["ch"], n_rx, sl["rx_stride"], sl["ch_stride"], sl["gsegs"], t["lv"], t["nv"], t["rec"], stream=s)
        m.ulsch_decode_symbols_device([dict(tb)], t["rec"], t["harq"], t["_out"], t["ack"], t["itm"], [sl["scr"]], stream=s)
    return Call(want, stage, issue)


# ---- the transport-block chain ---------------------------------------------------------------------------------------------------
TB = dict(A=valid_tbs(3000, 1), G=9600, BG=1, Qm=2, Nl=1, rv=0, tbslbrm=0)     # one segment, G > 2 A: every rv decodes on its own
TB6 = dict(A=valid_tbs(5000, 1), G=9600, BG=1, Qm=6, Nl=1, rv=0, tbslbrm=0)


def coded_want(tb, pay):
    co_end = (tb["G"] + 15) // 16 * 16 + 16
    return np.concatenate([O.dlsch_encode(tb, pay), np.full(co_end - tb["G"], CANARY8, np.uint8)])


def enc_calls(m, K):
    """dlsch_encode_device: variant k is redundancy version k of its own payload"""
    calls = []
    for k in range(K):
        tb, pay = dict(TB, rv=k), np.random.default_rng(610 + k).integers(0, 256, TB["A"] // 8, dtype=np.uint8)
        want = coded_want(tb, pay)
        calls.append(Call(dict(coded=want), lambda s, tb=tb, pay=pay, n=want.size: dict(pay=payload_dev(m, tb, pay), coded=fill(n, CANARY8, "uint8")),
                          lambda t, s, tb=tb: m.dlsch_encode_device([tb], t["pay"], t["coded"], stream=s)))
    return calls


def plan_calls(m, K):
    """the third call of a PreparedTbBatch: the plan is cached and nothing is uploaded.  Every batch has the same descriptors -- the
    thread finds one plan for all of them -- and its own payload.  stage() makes the first two calls on the batch's stream, waits
    for them and restores the canaries."""
    import torch
    calls = []
    for k in range(K):
        pay = np.random.default_rng(630 + k).integers(0, 256, TB["A"] // 8, dtype=np.uint8)
        want = coded_want(TB, pay)

        def stage(s, pay=pay, n=want.size):
            t = dict(pay=payload_dev(m, TB, pay), coded=fill(n, CANARY8, "uint8"), stream=s)
            t["batch"] = m.PreparedTbBatch([dict(TB)], t["pay"], t["coded"], stream=s)
            t["batch"].encode()
            t["batch"].encode()
            torch.cuda.synchronize()
            t["coded"].fill_(CANARY8)
            torch.cuda.synchronize()
            return t

        def issue(t, s):
            assert s == t["stream"]
            t["batch"].encode()
        calls.append(Call(dict(coded=want), stage, issue))
    return calls


def dec_calls(m, K):
    """ulsch_decode_device: variant k is redundancy version k of its own payload, received without noise"""
    calls = []
    for k in range(K):
        tb = dict(TB, rv=k, round=0, llrLen=0)
        pay = np.random.default_rng(650 + k).integers(0, 256, TB["A"] // 8, dtype=np.uint8)
        llr = ((1 - 2 * O.dlsch_encode(tb, pay).astype(np.int16)) * 20).astype(np.int16)
        want = decode_want(m, tb, llr)
        assert want["ack"][0] == 1 and np.array_equal(want["pay"], pay)
        calls.append(Call(want, lambda s, tb=tb, llr=llr, want=want: dict(decode_outputs(m, tb, want), llr=dev(np.concatenate([llr, np.zeros(32, np.int16)]))),
                          lambda t, s, tb=tb: m.ulsch_decode_device([dict(tb)], t["llr"], t["harq"], t["_out"], t["ack"], t["itm"], stream=s)))
    return calls


def decsym_calls(m, K):
    """ulsch_decode_symbols_device: variant k has its own payload, scrambling identity and noise"""
    calls = []
    for k in range(K):
        rng = np.random.default_rng(670 + k)
        tb = dict(TB6, round=0, llrLen=0)
        pay, scr = rng.integers(0, 256, tb["A"] // 8, dtype=np.uint8), (int(rng.integers(0, 0x10000)), 0, int(rng.integers(0, 1024)))
        _, y, mags = rx_inputs(rng, tb, scr_bits(tb, pay, scr)[1], 1.0)
        rec = m.pack_symbol_records([[y] + mags])[0]
        want = decode_want(m, tb, unscramble(demap_np(y, mags, tb["Qm"]), c_init_of(*scr), 0))
        assert want["ack"][0] == 1 and np.array_equal(want["pay"], pay)
        calls.append(Call(want, lambda s, tb=tb, rec=rec, want=want: dict(decode_outputs(m, tb, want), rec=dev(np.concatenate([rec, np.zeros(32, np.int16)]))),
                          lambda t, s, tb=tb, scr=scr: m.ulsch_decode_symbols_device([dict(tb)], t["rec"], t["harq"], t["_out"], t["ack"], t["itm"], [scr], stream=s)))
    return calls


BUILDERS = dict(pusch_channel_estimation=est_calls, pdsch_resource_mapping_precoded=map_calls, ulsch_mmse_2layers_grid=mmse_calls,
                dlsch_encode_symbols_device=encsym_calls, ulsch_decode_symbols_device=decsym_calls, cached_plan_encode=plan_calls,
                dlsch_encode_device=enc_calls, ulsch_decode_device=dec_calls)
# two strings of independent bits agree in half their places; every other output is many-valued
MOST = dict(dlsch_encode_device=0.4, cached_plan_encode=0.4)
