"""The estimator's measurements (max_ch, nvar) and the time average of its estimates, CPU only: the host forms
(nrLDPC_hip_pusch_chest_meas_host, nrLDPC_hip_pusch_chest_time_avg_host, nrLDPC_hip_pusch_chest_avg_segments) and the kernels of
csrc/tb_rx_chest_meas.hip run on the CPU (tests/emul/slot_chest_meas_emul.cpp) against the literal restatement of the reference's
loops (rx_chest_meas_np.py), bit for bit; the stand-alone sanitizer run of the emulation; and the refusals of the interface.

Misreadings of the reference that the cases notice (test_the_cases_notice_every_misreading runs the restatement with each of them
and requires that at least one case's result changes; the last is shown by calling twice on one set of arrays):
  max_after_cast     the TYPE1_INTERP maximum taken after the int16 cast instead of on the int32 LS value (:186-187)
  avg_edges          the first / last PRB included in the AVG modes' maximum (:295, :330 have no max_ch line)
  noise32            a 32-bit noise sum (:149 is a uint64_t)
  sat_sub            a saturating c16sub (tools_defs.h:186-191 casts: it wraps)
  t2_twice, t2_none  a TYPE2_INTERP pair counted by two 4-RE units, or by none (a pair straddles units)
  nest_per_antenna   nest_count per antenna instead of per call (:148 is outside the antenna loop)
  div_per_antenna    the division done per antenna (:468-469 is behind the antenna loop)
  div_after_sum      the division done after summing the descriptors (nr_ulsch_demodulation.c:1491 sums quotients)
  div_dmrs           nvar_div taken as the DMRS-symbol count (:1524 has nr_of_symbols)
  max_per_layer      max_ch not shared across a block's layers (:1470 is outside both loops)
  (not cleared)      accumulators that survive from one call to the next
For the time average (test_the_average_cases_notice_every_misreading): wide_sum (a wide sum, then a divide: the reference
saturates after every addition), shift3 (a multiply-and-shift for / 3), round_div (rounding division), reverse_order (the
symbols added in another order: saturation makes the order observable)."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rx_chest_meas_np as M
import rx_chest_np as R

ROOT = Path(__file__).resolve().parent.parent
EMUL = ROOT / "tests" / "emul"
CSRC = ROOT / "openairinterface5g_amd" / "csrc"
CLANG = "/opt/rocm/lib/llvm/bin/clang"
CXXFLAGS = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-pass-failed", "-Wno-unused-function", "-I", str(EMUL / "hip_host"), "-I", str(CSRC)]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g"]

T1I, T2I, T1A, T2A = 0, 1, 2, 3
FILL = 0x5a5a


# ---------------------------------------------------------------------------------------------------------
# the cases: a grid, descriptors, their blocks.  A descriptor: (mode, port, rb, k0, symbol, tb, layer)
# ---------------------------------------------------------------------------------------------------------
def _case(seed, N, n_rx, descs, blocks, delays=False, hot=False, n_sym_grid=None, ch_shift=0):
    """blocks = per tb (nr_of_symbols, nrOfLayers); the descriptors' estimates lie one after another from ch_shift on, the
    antennas' (and nothing else) ch_stride apart"""
    return dict(seed=seed, N=N, n_rx=n_rx, descs=descs, blocks=blocks, delays=delays, hot=hot, ch_shift=ch_shift,
                n_sym_grid=n_sym_grid or 1 + max(d[4] for d in descs))


CASES = {}
for _mode in (T1I, T2I, T1A, T2A):
    for _i, _rb in enumerate((1, 2, 3)):
        # rb_size 1, 2, 3 in every mode; n_rx 1, 2, 3, 4, 8 in turn; with and without delays
        _n_rx = (1, 2, 3, 4, 8)[(3 * _mode + _i) % 5]
        CASES[f"small-m{_mode}-rb{_rb}"] = _case(10 * _mode + _rb, 128, _n_rx, [(_mode, 0, _rb, 20, 0, 0, 0)], [(14, 1)], delays=_rb != 2, ch_shift=_rb)
    # more than one wave of units; the second layer's port has nushift / delta 1
    CASES[f"rb22-m{_mode}"] = _case(50 + _mode, 512, 2, [(_mode, 0, 22, 100, 0, 0, 0), (_mode, 2, 22, 100, 0, 0, 1)], [(12, 2)], delays=True, ch_shift=1)
    # an allocation across the grid's wrap (k0 even: nushift never reaches N)
    CASES[f"wrap-m{_mode}"] = _case(60 + _mode, 128, 3, [(_mode, 2 if _mode != T1I else 3, 5, 100, 0, 0, 0)], [(10, 1)], delays=bool(_mode & 1), ch_shift=2)
CASES["two-workgroups-t1i-rb86"] = _case(70, 1536, 1, [(T1I, 0, 86, 1000, 0, 0, 0)], [(14, 1)], delays=True)        # 258 units
CASES["second-piece-t1a-rb257"] = _case(71, 4096, 1, [(T1A, 0, 257, 3000, 0, 0, 0)], [(14, 1)])
# three blocks: interleaved descriptors; block 0 with 2 DMRS symbols x 2 layers; block 1 with no descriptor; block 2 another mode
CASES["three-blocks"] = _case(72, 256, 2, [(T1I, 0, 4, 30, 0, 0, 0), (T2I, 0, 3, 100, 1, 2, 0), (T1I, 2, 4, 30, 0, 0, 1), (T1I, 0, 4, 30, 2, 0, 0),
                                           (T2I, 2, 3, 100, 1, 2, 1), (T1I, 2, 4, 30, 2, 0, 1)], [(13, 2), (5, 1), (9, 2)], delays=True, ch_shift=3)
CASES["three-blocks-avg"] = _case(73, 256, 4, [(T2A, 0, 6, 30, 0, 0, 0), (T1A, 1, 5, 100, 1, 2, 0), (T2A, 1, 6, 30, 0, 0, 1)], [(13, 2), (5, 1), (9, 1)])
# a full-scale grid: the int32 LS value exceeds 32767 and one descriptor's noise_amp2 exceeds 2^32 (checked in the restatement)
CASES["full-scale-t1i"] = _case(74, 512, 4, [(T1I, 0, 22, 8, 0, 0, 0), (T1I, 2, 22, 8, 0, 0, 1)], [(4, 2)], hot=True)
CASES["full-scale-t2i"] = _case(75, 512, 2, [(T2I, 1, 22, 8, 0, 0, 0)], [(3, 1)], hot=True, delays=True)
# the cases the misreadings are tried on (the small and the structured ones: the restatement runs once per misreading)
MIS_CASES = [k for k in CASES if k.startswith(("small", "three", "full", "rb22-m1"))]


@functools.lru_cache(maxsize=None)
def build(name):
    """the arrays and descriptors of a case: rx int16 [n_rx, n_sym_grid N + 1, 2] (one c16 of slack for nothing: no read reaches it),
    segs, seg_tb, nvar_div, est_delay or None, ch layout"""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    N, n_rx = c["N"], c["n_rx"]
    L = c["n_sym_grid"] * N
    rx = (rng.choice([32767, -32767], (n_rx, L, 2)) if c["hot"] else rng.integers(-3000, 3001, (n_rx, L, 2))).astype(np.int16)
    segs, seg_tb, at = [], [], c["ch_shift"]
    for i, (mode, port, rb, k0, sym, tb, layer) in enumerate(c["descs"]):
        prb0 = 3 + i
        segs.append(dict(mode=mode, port=port, fft_size=N, start_re=k0, rb_size=rb, dmrs_offset=12 * prb0 // (3 if mode & 1 else 2),
                         c_init=R.c_init_pusch(3, sym, 40 + tb, tb & 1), rx_off=sym * N, ch_off=at, delay_off=i * n_rx))
        seg_tb.append(tb)
        at += 12 * rb + (i % 3)                                          # gaps of 0, 1, 2 c16: every alignment of the stores
    ch_stride = at + 1
    delays = rng.integers(-6, 7, len(segs) * n_rx).astype(np.int32) if c["delays"] else None
    nvar_div = [s * l * n_rx for s, l in c["blocks"]]
    return dict(c, rx=rx, rx_stride=L, segs=segs, seg_tb=seg_tb, nvar_div=nvar_div, est_delay=delays, ch_stride=ch_stride,
                ch_len=ch_stride * (n_rx - 1) + at)


@functools.lru_cache(maxsize=None)
def restated(name, mis=()):
    """-> (max_ch per block, nvar per block, the whole ul_ch array as the call leaves one filled with FILL, per-descriptor
    (max_ch from 0, noise_amp2, nest_count))"""
    b = build(name)
    ants = [[(int(r), int(i)) for r, i in b["rx"][a]] for a in range(b["n_rx"])]
    ch = np.full((b["ch_len"], 2), FILL, np.int16)
    max_ch, nvar, per_desc = [], [], {}
    for tb, (n_symbols, layers) in enumerate(b["blocks"]):
        idx = [i for i, t in enumerate(b["seg_tb"]) if t == tb]
        calls = []
        for i in idx:
            s, d = b["segs"][i], b["descs"][i]
            dl = [int(b["est_delay"][s["delay_off"] + a]) if b["est_delay"] is not None else 0 for a in range(b["n_rx"])]
            calls.append(dict(rx_ants=ants, soffset=s["rx_off"], N=b["N"], k0=s["start_re"], nb_rb=s["rb_size"], p=s["port"], dmrs_type=s["mode"] & 1,
                              chest_freq=s["mode"] >> 1, c_init=s["c_init"], re_offset=12 * (3 + i), est_delays=dl, layer=d[6]))
        n_dmrs = len({b["descs"][i][4] for i in idx})
        m, v, ul = M.pdu_measurements(calls, n_symbols, layers, b["n_rx"], n_dmrs=max(n_dmrs, 1), mis=frozenset(mis))
        max_ch.append(m)
        nvar.append(v)
        for i, c, u in zip(idx, calls, ul):
            args = {k: x for k, x in c.items() if k != "layer"}
            if not mis:
                r = M.estimation_call(max_ch=0, **args)
                per_desc[i] = (r[0], r[2], r[3])
            for a in range(b["n_rx"]):
                o = b["segs"][i]["ch_off"] + a * b["ch_stride"]
                ch[o:o + 12 * b["segs"][i]["rb_size"]] = np.array(u[a], np.int64).astype(np.int16)
    return max_ch, nvar, ch, per_desc


# ---------------------------------------------------------------------------------------------------------
# the emulated kernels
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    import openairinterface5g_amd.ldpc as m
    so = tmp_path_factory.mktemp("chest_meas_emul") / "libchest_meas_emul.so"
    subprocess.run([CLANG + "++", "-O2", "-fPIC", "-shared", *CXXFLAGS, "-o", str(so), str(EMUL / "slot_chest_meas_emul.cpp"), "-lpthread"], check=True)
    L = C.CDLL(str(so))
    L.slot_chest_meas_emul_last_error.restype = C.c_char_p
    U = C.POINTER(C.c_uint32)
    L.slot_emul_pusch_channel_estimation_meas.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(m.nrLDPC_hip_chest_seg_t),
                                                          C.c_uint32, C.c_void_p, U, U, C.c_uint32, C.c_void_p, C.c_void_p]
    L.slot_emul_pusch_chest_time_avg.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(m.nrLDPC_hip_chest_avg_seg_t), C.c_uint32]
    return L


def emul_meas(L, b, ch, max_ch, nvar):
    import openairinterface5g_amd.ldpc as m
    rc = L.slot_emul_pusch_channel_estimation_meas(b["rx"].ctypes.data, b["rx_stride"], ch.ctypes.data, b["ch_stride"], b["n_rx"],
                                                   m._chest_seg_array(b["segs"]), len(b["segs"]),
                                                   None if b["est_delay"] is None else b["est_delay"].ctypes.data, m._u32_array(b["seg_tb"]),
                                                   m._u32_array(b["nvar_div"]), len(b["nvar_div"]), max_ch.ctypes.data, nvar.ctypes.data)
    assert rc == 0, L.slot_chest_meas_emul_last_error()


def test_the_full_scale_case_is_one(built):
    """what the case is for, established in the restatement: an LS value beyond int16 and a noise sum beyond 32 bits"""
    max_ch, _, _, per_desc = restated("full-scale-t1i")
    assert max_ch[0] > 32767
    assert max(noise for _, noise, _ in per_desc.values()) > 2 ** 32
    assert all(nest == 12 * 22 * 4 for _, _, nest in per_desc.values())


def test_the_cases_notice_every_misreading(built):
    for mis in M.MISREADINGS:
        changed = [k for k in MIS_CASES if restated(k, (mis,))[:2] != restated(k)[:2]]
        assert changed, mis


@pytest.mark.parametrize("name", list(CASES))
def test_host_form_equals_the_restatement(built, name):
    import openairinterface5g_amd.ldpc as m
    b = build(name)
    max_ch, nvar, _, per_desc = restated(name)
    got_max, got_nvar = [0] * len(b["blocks"]), [0] * len(b["blocks"])
    for i, s in enumerate(b["segs"]):
        mx, noise, nest = m.pusch_chest_meas_host(b["rx"], b["rx_stride"], b["n_rx"], s, b["est_delay"])
        assert (mx, noise, nest) == per_desc[i], (name, i)
        tb = b["seg_tb"][i]
        got_max[tb] = max(got_max[tb], mx)
        got_nvar[tb] = (got_nvar[tb] + (noise // nest if nest else 0)) & 0xffffffff
    assert got_max == max_ch and [v // d for v, d in zip(got_nvar, b["nvar_div"])] == nvar, name


@pytest.mark.parametrize("name", list(CASES))
def test_emulated_kernels_equal_the_restatement(built, emul, name):
    b = build(name)
    max_ch, nvar, want_ch, _ = restated(name)
    n_tb = len(b["blocks"])
    ch = np.full((b["ch_len"], 2), FILL, np.int16)
    for rep in range(2):                                                 # the same call twice on one set of arrays
        got_max, got_nvar = np.full(n_tb, -1, np.int32), np.full(n_tb, 0xffffffff, np.uint32)
        emul_meas(emul, b, ch, got_max, got_nvar)
        assert got_max.tolist() == max_ch and got_nvar.tolist() == nvar, (name, rep)
        assert np.array_equal(ch, want_ch), (name, rep)                  # the estimates and nothing but the write set


def test_blocks_without_any_descriptor(built, emul):
    """a call with blocks and no descriptor at all: 0 / 0 for each, in the emulated kernels and in HOST mem (which needs no GPU for it)"""
    import openairinterface5g_amd.ldpc as m
    b = dict(build("small-m0-rb1"), segs=[], seg_tb=[], nvar_div=[3, 9], est_delay=None)
    ch = np.full((b["ch_len"], 2), FILL, np.int16)
    mx, nv = np.full(2, -1, np.int32), np.full(2, 0xffffffff, np.uint32)
    emul_meas(emul, b, ch, mx, nv)
    assert mx.tolist() == [0, 0] and nv.tolist() == [0, 0] and np.all(ch == FILL)
    _, mx, nv = m.pusch_channel_estimation_meas(b["rx"].reshape(-1, 2), b["rx_stride"], ch, b["ch_stride"], b["n_rx"], [], [], [3, 9])
    assert mx.tolist() == [0, 0] and nv.tolist() == [0, 0] and np.all(ch == FILL)


# ---------------------------------------------------------------------------------------------------------
# the rank-2 slots of ul_slot_np.py with the measured values in the receivers' place of the true ones
# ---------------------------------------------------------------------------------------------------------
# The MMSE receiver (256QAM, four antennas) and the ML receiver (QPSK, two).  Of the four MMSE slots of ul_slot_np.py the two averaging
# ones measure nvar = 0 (nest_count stays 0) and decode; "2L-T1I" measures 29 against the noise model's 18 and decodes; "2L-T2I" does
# not decode with the measured value: with ports 0 and 1 on one CDM group ch0 - ch of nr_ul_channel_estimation.c:273 is half the
# difference of the pair's two products, which is the other layer's channel, so the reference's nvar there is that layer's power
# (7724 on that slot) and not the noise.  That is the reference's arithmetic, restated and built as written.
E2E_SLOTS = ("2L-T1I", "2L-T1I-ml4")


@functools.lru_cache(maxsize=None)
def slot_measured(name):
    """(the slot, its seg_tb, nvar_div, restated max_ch, restated nvar): both layers' descriptors are block 0's"""
    import openairinterface5g_amd.ldpc as m
    import ul_slot_np as U
    sl = U.slot_of(m, name)
    c, a = sl["case"], sl["alloc"]
    ants = [[(int(r), int(i)) for r, i in sl["rx"][k]] for k in range(c["n_rx"])]
    calls = [dict(rx_ants=ants, soffset=s["rx_off"], N=c["N"], k0=s["start_re"], nb_rb=s["rb_size"], p=s["port"], dmrs_type=s["mode"] & 1,
                  chest_freq=s["mode"] >> 1, c_init=s["c_init"], re_offset=12 * (a["bwp_start"] + a["rb_start"]),
                  est_delays=[int(sl["delay"][s["delay_off"] + k]) for k in range(c["n_rx"])], layer=l) for l, s in enumerate(sl["csegs"])]
    max_ch, nvar, _ = M.pdu_measurements(calls, a["nr_of_symbols"], c["n_layers"], c["n_rx"])
    return sl, [0] * len(sl["csegs"]), [a["nr_of_symbols"] * c["n_layers"] * c["n_rx"]], max_ch, nvar


@pytest.mark.parametrize("name", E2E_SLOTS)
def test_the_rank2_slots_decode_with_the_measured_values(built, name):
    """established on the CPU before the GPU test relies on it: the numpy receivers fed the restated max_ch / nvar, the oracle's
    decoder behind them (as test_ul_slot_host.py does with the true channel's values)"""
    import openairinterface5g_amd.ldpc as m
    import ul_slot_np as U
    sl, _, _, max_ch, nvar = slot_measured(name)
    assert 0 < max_ch < 2048                                             # shift_ch_ext stays 0, as with the true channel's maximum
    lv, rec = U.front_records(dict(sl, max_ch=max_ch, nvar=nvar), U.estimate_host(m, sl), None)
    got, ack, iters = U.decode_record(sl, rec)
    assert ack and np.array_equal(got, sl["pay"]), (name, max_ch, nvar, iters)


# ---------------------------------------------------------------------------------------------------------
# the time average
# ---------------------------------------------------------------------------------------------------------
def avg_case(n_sym, rb, shift, n_plane, seed=0):
    """symbols 12 rb + 5 apart (every symbol at another alignment), planes stride apart; values that saturate on the second addition
    but not on the first, and negative sums for / 3"""
    rng = np.random.default_rng(1000 * n_sym + 10 * rb + shift + seed)
    gap = 12 * rb + 5
    stride = 4 * gap + 1
    n = shift + (n_plane - 1) * stride + (n_sym - 1) * gap + 12 * rb
    ch = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
    seg = dict(ch_off=[shift + s * gap for s in range(n_sym)], n_sym=n_sym, rb_size=rb)
    if n_sym >= 3:
        for q in range(n_plane):
            o = [c + q * stride for c in seg["ch_off"]]
            ch[o[0]], ch[o[1]], ch[o[2]] = (12000, -12000), (12000, -12000), (12000, -12000)      # 24000, then 32767 / -32768
            ch[o[0] + 1], ch[o[1] + 1], ch[o[2] + 1] = (30000, -30000), (30000, -30000), (-30000, 30000)   # the order shows
            ch[o[0] + 2], ch[o[1] + 2], ch[o[2] + 2] = (-5, -1), (-3, 0), (-3, -1)                # -11 / 3 = -3, not -4
    return ch, seg, stride


def avg_restated(ch, seg, stride, n_plane, mis=()):
    out = ch.copy()
    for q in range(n_plane):
        syms = [[(int(r), int(i)) for r, i in ch[o + q * stride:o + q * stride + 12 * seg["rb_size"]]] for o in seg["ch_off"]]
        o = seg["ch_off"][0] + q * stride
        out[o:o + 12 * seg["rb_size"]] = np.array(M.chest_time_domain_avg(syms, frozenset(mis)), np.int64).astype(np.int16)
    return out


AVG_CASES = [(n_sym, rb, shift, 2 + 2 * (shift & 1)) for n_sym in (1, 2, 3, 4) for rb in (1, 5, 22) for shift in range(4)]


def test_the_average_cases_notice_every_misreading():
    for mis in M.AVG_MISREADINGS:
        assert any(not np.array_equal(avg_restated(*avg_case(*c[:3], c[3]), c[3], (mis,)), avg_restated(*avg_case(*c[:3], c[3]), c[3]))
                   for c in AVG_CASES if c[1] == 5), mis


def test_time_average_host_form_and_emulated_kernel(built, emul):
    import openairinterface5g_amd.ldpc as m
    for n_sym, rb, shift, n_plane in AVG_CASES:
        ch, seg, stride = avg_case(n_sym, rb, shift, n_plane)
        want = avg_restated(ch, seg, stride, n_plane)
        if n_sym == 1:
            assert np.array_equal(want, ch)
        host = ch.copy()
        for q in range(n_plane):
            m.pusch_chest_time_avg_host(host, dict(seg, ch_off=[o + q * stride for o in seg["ch_off"]]))
        assert np.array_equal(host, want), (n_sym, rb, shift)
        got = ch.copy()
        assert emul.slot_emul_pusch_chest_time_avg(got.ctypes.data, stride, n_plane, m._chest_avg_seg_array([seg]), 1) == 0
        assert np.array_equal(got, want), (n_sym, rb, shift)                    # the whole array: the other symbols stay


def alloc(**kw):
    a = dict(tb=0, Qm=2, dmrs_config_type=0, num_dmrs_cdm_grps_no_data=2, dmrs_symbol=2, fft_size=512, first_carrier_offset=100, bwp_start=0, rb_start=3,
             rb_size=10, start_symbol=1, nr_of_symbols=12, ul_dmrs_symb_pos=0, plane=1 << 20, rx_slot_off=0, ch_off=7, rec_off=0)
    a.update(kw)
    return a


def test_avg_segments(built):
    import openairinterface5g_amd.ldpc as m
    # a DMRS bit outside the allocation's symbols does not count
    segs, first = m.pusch_chest_avg_segments([alloc(ul_dmrs_symb_pos=(1 << 0) | (1 << 2) | (1 << 7) | (1 << 11) | (1 << 13)), alloc(ul_dmrs_symb_pos=1 << 5, ch_off=9000)])
    assert segs == [dict(ch_off=[7 + 2 * 512, 7 + 7 * 512, 7 + 11 * 512], n_sym=3, rb_size=10), dict(ch_off=[9000 + 5 * 512], n_sym=1, rb_size=10)]
    assert first == [2, 5]
    for bad, text in ((alloc(ul_dmrs_symb_pos=0b101010101010), "more than four"), (alloc(ul_dmrs_symb_pos=1 << 0), "no DMRS symbol"),
                      (alloc(nr_of_symbols=14), "within the slot"), (alloc(rb_size=0), "rb_size is 0")):
        with pytest.raises(RuntimeError, match=text):
            m.pusch_chest_avg_segments([bad])
    with pytest.raises(RuntimeError, match="more descriptors than cap"):
        m.pusch_chest_avg_segments([alloc(ul_dmrs_symb_pos=4), alloc(ul_dmrs_symb_pos=4)], cap=1)


# ---------------------------------------------------------------------------------------------------------
# refusals (they come before anything is enqueued or written, so HOST mem shows them without a GPU)
# ---------------------------------------------------------------------------------------------------------
def test_meas_refusals(built):
    import openairinterface5g_amd.ldpc as m
    b = build("three-blocks")
    ch = np.full((b["ch_len"], 2), FILL, np.int16)

    def call(segs=b["segs"], seg_tb=b["seg_tb"], nvar_div=b["nvar_div"], n_rx=b["n_rx"], ch_stride=b["ch_stride"]):
        m.pusch_channel_estimation_meas(b["rx"], b["rx_stride"], ch, ch_stride, n_rx, segs, seg_tb, nvar_div, b["est_delay"])
    with pytest.raises(RuntimeError, match="seg_tb names a block >= n_tb"):
        call(seg_tb=[0, 3, 0, 0, 2, 0])
    with pytest.raises(RuntimeError, match="nvar_div is 0"):
        call(nvar_div=[5, 0, 7])
    # everything the plain call refuses
    with pytest.raises(RuntimeError, match="n_rx must be 1..8"):
        call(n_rx=0)
    with pytest.raises(RuntimeError, match="mode must be"):
        call(segs=[dict(b["segs"][0], mode=4)] + b["segs"][1:])
    with pytest.raises(RuntimeError, match="overlap"):
        call(segs=[b["segs"][0], dict(b["segs"][1], ch_off=b["segs"][0]["ch_off"] + 3)] + b["segs"][2:])
    with pytest.raises(RuntimeError, match="rb_size is 0"):
        call(segs=[dict(b["segs"][0], rb_size=0)] + b["segs"][1:])
    # NULL arrays, and another mem value, through the C interface
    L = m._chest_meas_lib()
    segs, tb, div = m._chest_seg_array(b["segs"]), m._u32_array(b["seg_tb"]), m._u32_array(b["nvar_div"])
    mx, nv = np.zeros(3, np.int32), np.zeros(3, np.uint32)
    args = [b["rx"].ctypes.data, b["rx_stride"], ch.ctypes.data, b["ch_stride"], b["n_rx"], segs, 6, None, tb, div, 3, mx.ctypes.data, nv.ctypes.data,
            m.MEM_HOST, None]
    for k in (0, 2, 5, 8, 9, 11, 12):
        a = list(args)
        a[k] = None
        assert L.nrLDPC_hip_pusch_channel_estimation_meas(*a) != 0 and "null argument" in m.last_error(), k
    assert L.nrLDPC_hip_pusch_channel_estimation_meas(*args[:13], 7, None) != 0 and "mem must be" in m.last_error()
    assert np.all(ch == FILL) and not mx.any() and not nv.any()                  # nothing was written
    # the host form
    for k in (0, 3, 5, 6, 7):
        a = [b["rx"].ctypes.data, b["rx_stride"], b["n_rx"], segs, None, C.byref(C.c_int32()), C.byref(C.c_uint64()), C.byref(C.c_uint32())]
        a[k] = None
        assert L.nrLDPC_hip_pusch_chest_meas_host(*a) != 0 and "null argument" in m.last_error(), k
    with pytest.raises(RuntimeError, match="n_rx must be 1..8"):
        m.pusch_chest_meas_host(b["rx"], 0, 0, b["segs"][0])
    with pytest.raises(RuntimeError, match="port must be"):
        m.pusch_chest_meas_host(b["rx"], b["rx_stride"], 2, dict(b["segs"][0], port=8))


def test_time_avg_refusals(built):
    import openairinterface5g_amd.ldpc as m
    ch = np.zeros((4000, 2), np.int16)
    ok = dict(ch_off=[0, 100, 200], n_sym=3, rb_size=5)
    for seg, n_plane, stride, text in ((dict(ok, n_sym=0), 2, 1000, "n_sym must be 1..4"), (dict(ok, n_sym=5, ch_off=[0, 100, 200, 300]), 2, 1000, "n_sym must be 1..4"),
                                       (dict(ok, rb_size=0), 2, 1000, "rb_size must be"), (ok, 0, 1000, "n_plane must be 1..16"),
                                       (ok, 17, 10, "n_plane must be 1..16"), (ok, 2, 30, "write ranges of two"),
                                       (dict(ok, ch_off=[0, 30, 200]), 1, 1000, "overlaps a range that is written"),
                                       (ok, 2, 100, "overlaps a range that is written")):
        with pytest.raises(RuntimeError, match=text):
            m.pusch_chest_time_avg(ch, stride, n_plane, [seg])
    with pytest.raises(RuntimeError, match="write ranges of two"):
        m.pusch_chest_time_avg(ch, 1000, 1, [ok, dict(ok, ch_off=[59, 400, 500])])
    with pytest.raises(RuntimeError, match="n_sym must be 1..4"):
        m.pusch_chest_time_avg_host(ch, dict(ok, n_sym=5, ch_off=[0, 100, 200, 300]))
    L = m._chest_meas_lib()
    arr = m._chest_avg_seg_array([ok])
    assert L.nrLDPC_hip_pusch_chest_time_avg(None, 1000, 1, arr, 1, m.MEM_HOST, None) != 0 and "null argument" in m.last_error()
    assert L.nrLDPC_hip_pusch_chest_time_avg(ch.ctypes.data, 1000, 1, None, 1, m.MEM_HOST, None) != 0 and "null argument" in m.last_error()
    assert L.nrLDPC_hip_pusch_chest_time_avg(ch.ctypes.data, 1000, 1, arr, 1, 9, None) != 0 and "mem must be" in m.last_error()
    assert L.nrLDPC_hip_pusch_chest_time_avg_host(None, arr) != 0 and "null argument" in m.last_error()
    assert not ch.any()
    # n_sym = 1 reads and writes nothing: no GPU is needed for it
    m.pusch_chest_time_avg(ch, 1000, 2, [dict(ch_off=[3], n_sym=1, rb_size=5)])
    assert not ch.any()


# ---------------------------------------------------------------------------------------------------------
# the emulated kernels under the host sanitizers, on arrays of exactly the documented extents
# ---------------------------------------------------------------------------------------------------------
def test_emulated_kernels_on_exact_buffers_under_the_host_sanitizers(tmp_path):
    """a stand-alone program (its own main): sanitized code is never loaded into Python.  DESIGN.md 4.15"""
    jobs = [subprocess.Popen([CLANG, *SAN, "-c", str(CSRC / "nr_coding_host.c"), "-o", str(tmp_path / "nr_coding_host.o")]),
            subprocess.Popen([CLANG + "++", *SAN, *CXXFLAGS, "-DCHEST_MEAS_EMUL_MAIN", "-c", str(EMUL / "slot_chest_meas_emul.cpp"), "-o",
                              str(tmp_path / "slot_chest_meas_emul.o")])]
    assert [j.wait() for j in jobs] == [0, 0]
    exe = tmp_path / "chest_meas_emul_san"
    subprocess.run([CLANG + "++", *SAN, "-o", str(exe), str(tmp_path / "nr_coding_host.o"), str(tmp_path / "slot_chest_meas_emul.o"), "-lpthread"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-4000:]
    calls, bad = (int(x) for x in r.stdout.split())
    assert calls > 100 and bad == 0, r.stdout
