"""The slot-level kernels' thread-to-element decomposition on the CPU (tests/emul/slot_rx_emul.cpp, slot_tx_emul.cpp, slot_scr_emul.cpp): the .hip
files themselves, read against the host shim (tests/emul/hip_host/), run over the plans the library builds (csrc/*_plan.h) on the
cases of the GPU tests -- the builders are imported, not copied -- in place on canary-filled arrays, as a DEVICE mem call does.  The
results must equal the host forms (the *_host calls, which go element by element and share none of the decomposition) bit for bit;
no tolerance anywhere.  What this proves and what it does not: DESIGN.md 4.15.  The same kernels on arrays of exactly the
documented extents under AddressSanitizer: test_slot_kernels_san.py."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import test_gpu_dl_symbols as GDS
import test_gpu_pdsch_map as GPM
import test_gpu_pdsch_precode as GPP
import test_gpu_qam as GQ
import test_gpu_rx_chest as GCH
import test_gpu_rx_front as GRF
import test_gpu_rx_grid as GRG
import test_gpu_rx_mmse as GRM
import test_gpu_scrambling as GS
from layer_np import layer_map_np
from qam_np import demap_np, edge_symbols, modulate_np
from rx_front_np import level_np
from rx_mmse_np import level_mmse_np, records_np
from test_scrambling_host import c_init_of

ROOT = Path(__file__).resolve().parent.parent
CANARY = 0x5a5a
P, U32, U64 = C.c_void_p, C.c_uint32, C.c_uint64


@pytest.fixture(scope="module")
def emul(built):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    L = C.CDLL(str(ROOT / "tests" / "emul" / "libslot_emul.so"))
    L.slot_emul_last_error.restype = C.c_char_p
    sigs = {
        "slot_emul_channel_compensation": [P, P, U32, U64, C.POINTER(m.nrLDPC_hip_rx_seg_t), U32, P, P],
        "slot_emul_channel_level": [P, U32, U64, C.POINTER(m.nrLDPC_hip_rx_seg_t), U32, P],
        "slot_emul_channel_compensation_grid": [P, P, U32, U64, U64, C.POINTER(m.nrLDPC_hip_rx_grid_seg_t), U32, P, P],
        "slot_emul_channel_level_grid": [P, U32, U64, C.POINTER(m.nrLDPC_hip_rx_grid_seg_t), U32, P],
        "slot_emul_mmse_2layers_grid": [P, P, U32, U64, U64, C.POINTER(m.nrLDPC_hip_rx_grid_seg_t), U32, P, P, P],
        "slot_emul_channel_level_grid_mmse": [P, U32, U64, C.POINTER(m.nrLDPC_hip_rx_grid_seg_t), U32, P, P],
        "slot_emul_pusch_channel_estimation": [P, U64, P, U64, U32, C.POINTER(m.nrLDPC_hip_chest_seg_t), U32, P],
        "slot_emul_pdsch_resource_mapping": [P, P, U64, U32, C.POINTER(m.nrLDPC_hip_pdsch_map_seg_t), U32],
        "slot_emul_pdsch_resource_mapping_precoded": [P, P, U64, U32, C.POINTER(m.nrLDPC_hip_pdsch_map_seg_t), C.POINTER(m.nrLDPC_hip_pdsch_prg_t), U32, P,
                                                      U32, C.POINTER(m.nrLDPC_hip_pm_pdu_t), U32],
        "slot_emul_modulation": [P, U32, U32, P],
        "slot_emul_ulsch_llr": [P, P, P, P, U32, U32, P],
        "slot_emul_layer_mapping": [P, U32, U32, P, U32],
        "slot_emul_scramble_map_tb": [P, U32, U32, P, P],
        "slot_emul_scramble_bits": [P, U32, U32, P],
        "slot_emul_unscramble_llr": [P, U32, U32],
        "slot_emul_scramble_bits_tb": [P, U32, U32, P, P],
    }
    for name, args in sigs.items():
        getattr(L, name).argtypes = args
        getattr(L, name).restype = C.c_int32
    return L, m


def ok(L, rc):
    assert rc == 0, L.slot_emul_last_error().decode()


def aligned16(n, dtype, fill):
    """n elements that begin at a 16-byte aligned address: the pads below then give the 4- and 8-byte aligned cases"""
    raw = np.empty(n * np.dtype(dtype).itemsize + 16, np.uint8)
    a = raw[(-raw.ctypes.data) % 16:][:n * np.dtype(dtype).itemsize].view(dtype)
    a[:] = fill
    assert a.ctypes.data % 16 == 0
    return a


def records_in_place(want, call):
    """the record array 16-, 4- and 8-byte aligned, canaries on both sides"""
    for pad in (0, 2, 4):
        rec = aligned16(want.size + 8, np.int16, CANARY)
        call(rec[pad:].ctypes.data)
        assert (rec[:pad] == CANARY).all() and (rec[pad + want.size:] == CANARY).all()
        assert np.array_equal(rec[pad:pad + want.size], want), (pad, np.flatnonzero(rec[pad:pad + want.size] != want)[:8])


# ---- the single-layer front on extracted arrays (tb_rx_front.hip) -----------------------------------------------------------
@pytest.mark.parametrize("n_rx", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("Qm", [2, 4, 6, 8])
def test_compensation_and_level(emul, Qm, n_rx):
    L, m = emul
    rng = np.random.default_rng(1000 * Qm + n_rx)
    segs, rx, ch, stride, shift, want = GRF.kernel_case(rng, Qm, n_rx)
    host = np.full(want.size, CANARY, np.int16)
    for s in segs:
        nb = s["nb_re"]
        planes = m.ulsch_compensate_host(rx[:, s["rx_off"]:s["rx_off"] + nb], ch[:, s["ch_off"]:s["ch_off"] + nb], n_rx, nb, nb, Qm, int(shift[s["tb"]]))
        for k in range(Qm // 2):
            o = s["rec_off"] + 2 * (k * s["plane"] + s["sym_off"])
            host[o:o + 2 * nb] = planes[k].reshape(-1)
    assert np.array_equal(host, want)
    rx0, ch0 = rx.copy(), ch.copy()
    arr = m._rx_seg_array(segs)
    records_in_place(want, lambda rec: ok(L, L.slot_emul_channel_compensation(rx.ctypes.data, ch.ctypes.data, n_rx, stride, arr, len(segs),
                                                                              shift.ctypes.data, rec)))
    n_blocks = len(shift)
    first = [next(s for s in segs if s["tb"] == b) for b in range(n_blocks)][::-1]
    lv_want = [m.ulsch_level_host(np.ascontiguousarray(ch[:, s["ch_off"]:s["ch_off"] + s["nb_re"]]), n_rx, s["nb_re"], s["nb_re"])[0] for s in first[::-1]]
    assert lv_want == [level_np(ch[:, s["ch_off"]:s["ch_off"] + s["nb_re"]])[0] for s in first[::-1]]
    lv = np.full(n_blocks + 2, -7, np.int32)
    ok(L, L.slot_emul_channel_level(ch.ctypes.data, n_rx, stride, m._rx_seg_array(first), n_blocks, lv.ctypes.data))
    assert lv.tolist() == lv_want + [-7, -7]
    assert np.array_equal(rx, rx0) and np.array_equal(ch, ch0)


# ---- the same from the OFDM grid -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rx,Qm", GRG.GRID_PARAMS)
def test_grid_compensation_and_level(emul, n_rx, Qm):
    L, m = emul
    rng = np.random.default_rng(2000 * Qm + n_rx)
    segs, ext_segs, rx, ch, rx_stride, ch_stride, rx_e, ch_e, shift, want = GRG.grid_case(rng, Qm, n_rx)
    n_ext = rx_e.shape[1]
    host = np.full(want.size, CANARY, np.int16)
    for s, e in zip(segs, ext_segs):                                     # extract_host, then compensate_host
        nb = s["nb_re"]
        for a in range(n_rx):
            xa, ca = m.ulsch_extract_host(rx[a, s["rx_off"]:], ch[a, s["ch_off"]:], s["pattern"], s["fft_size"], s["start_re"], nb)
            assert np.array_equal(xa, rx_e[a, e["rx_off"]:e["rx_off"] + nb]) and np.array_equal(ca, ch_e[a, e["ch_off"]:e["ch_off"] + nb])
        planes = m.ulsch_compensate_host(rx_e[:, e["rx_off"]:], ch_e[:, e["ch_off"]:], n_rx, n_ext - e["rx_off"], nb, Qm, int(shift[s["tb"]]))
        for k in range(Qm // 2):
            o = s["rec_off"] + 2 * (k * s["plane"] + s["sym_off"])
            host[o:o + 2 * nb] = planes[k].reshape(-1)
    assert np.array_equal(host, want)
    rx0, ch0 = rx.copy(), ch.copy()
    arr = m._rx_grid_seg_array(segs)
    records_in_place(want, lambda rec: ok(L, L.slot_emul_channel_compensation_grid(rx.ctypes.data, ch.ctypes.data, n_rx, rx_stride, ch_stride, arr,
                                                                                   len(segs), shift.ctypes.data, rec)))
    fi = GRG.measurement_symbols(segs, n_rx)
    lv_want = [m.ulsch_level_host(np.ascontiguousarray(GRG.extract_np(rx, ch, segs[i])[1]), n_rx, segs[i]["nb_re"], segs[i]["nb_re"])[0] for i in fi[::-1]]
    lv = np.full(4, -7, np.int32)
    ok(L, L.slot_emul_channel_level_grid(ch.ctypes.data, n_rx, ch_stride, m._rx_grid_seg_array([segs[i] for i in fi]), 2, lv.ctypes.data))
    assert lv.tolist() == lv_want + [-7, -7]
    assert np.array_equal(rx, rx0) and np.array_equal(ch, ch0)


# ---- the two-layer MMSE receiver (tb_rx_mmse.hip) ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_rx,Qm", [(2, 6), (4, 6), (2, 8), (4, 8)])
def test_mmse_grid(emul, n_rx, Qm):
    L, m = emul
    rng = np.random.default_rng(3000 * Qm + n_rx)
    segs, rx, ch, rx_stride, ch_stride, shift, nvar, want = GRM.grid_case(rng, Qm, n_rx)
    host = np.full(want.size, CANARY, np.int16)
    for s in segs:
        a, b = GRM.pairs_np(rx, ch, s, n_rx)
        got = m.ulsch_mmse_2layers_host(np.ascontiguousarray(a), np.ascontiguousarray(b.reshape(2 * n_rx, s["nb_re"], 2)), n_rx, s["nb_re"], s["nb_re"], Qm,
                                        int(shift[s["tb"]]), int(nvar[s["tb"]]))
        records_np(host, got, Qm, s["plane"], s["sym_off"], s["rec_off"])
    assert np.array_equal(host, want)
    rx0, ch0 = rx.copy(), ch.copy()
    arr = m._rx_grid_seg_array(segs)
    records_in_place(want, lambda rec: ok(L, L.slot_emul_mmse_2layers_grid(rx.ctypes.data, ch.ctypes.data, n_rx, rx_stride, ch_stride, arr, len(segs),
                                                                           shift.ctypes.data, nvar.ctypes.data, rec)))
    assert np.array_equal(rx, rx0) and np.array_equal(ch, ch0)


@pytest.mark.parametrize("n_rx", [2, 4])
def test_level_grid_mmse(emul, n_rx):
    L, m = emul
    ch, cs, first, max_ch = GRM.level_case(n_rx)
    want = [0, 0, 0]
    for f in first:
        pairs = np.ascontiguousarray(GRG.extract_np(ch[:1], ch, f)[1])
        want[f["tb"]] = m.ulsch_level_mmse_host(pairs, n_rx, f["nb_re"], f["nb_re"], int(max_ch[f["tb"]]))[0]
        assert want[f["tb"]] == level_mmse_np(pairs.reshape(2, n_rx, f["nb_re"], 2), int(max_ch[f["tb"]]))[0]
    assert len(set(want)) > 1
    lv = np.full(5, -7, np.int32)
    ok(L, L.slot_emul_channel_level_grid_mmse(ch.ctypes.data, n_rx, cs, m._rx_grid_seg_array(first), 3, max_ch.ctypes.data, lv.ctypes.data))
    assert lv.tolist() == want + [-7, -7]


# ---- PUSCH DMRS channel estimation (tb_rx_chest.hip) -------------------------------------------------------------------------
@pytest.mark.parametrize("n_rx", [1, 2, 3, 4])
def test_channel_estimation(emul, n_rx):
    L, m = emul
    rng = np.random.default_rng(50 + n_rx)
    segs, rx, rs, cs, delay = GCH.mixed_case(rng, n_rx)
    arr = m._chest_seg_array(segs)
    for dl in (delay, None):
        want = GCH.host_form(m, segs, rx, rs, cs, n_rx, dl)
        written = want != CANARY
        assert written.any() and not written.all()
        for pad in (0, 1, 2, 3):                                         # the estimates 16-, 4-, 8- and 12-byte aligned
            ch = aligned16(2 * (n_rx * cs + 4), np.int16, CANARY)
            ok(L, L.slot_emul_pusch_channel_estimation(rx.ctypes.data, rs, ch[2 * pad:].ctypes.data, cs, n_rx, arr, len(segs),
                                                       None if dl is None else dl.ctypes.data))
            got = ch.reshape(-1, 2)
            assert (got[:pad] == CANARY).all() and (got[pad + n_rx * cs:] == CANARY).all()
            assert np.array_equal(got[pad:pad + n_rx * cs], want), (n_rx, pad, np.argwhere(got[pad:pad + n_rx * cs] != want)[:4])


# ---- PDSCH resource mapping, unit and precoded (tb_tx_map.hip) ----------------------------------------------------------------
def grid_in_place(want, n_tx, stride, call):
    """the transmit grid 16-, 4-, 8- and 12-byte aligned (the phase of every antenna's groups moves with it), canaries on both sides"""
    for pad in (0, 1, 2, 3):
        tx = aligned16(2 * (n_tx * stride + 4), np.int16, CANARY)
        call(tx[2 * pad:].ctypes.data)
        got = tx.reshape(-1, 2)
        assert (got[:pad] == CANARY).all() and (got[pad + n_tx * stride:] == CANARY).all()
        assert np.array_equal(got[pad:pad + n_tx * stride], want), (pad, np.argwhere(got[pad:pad + n_tx * stride] != want)[:4])


@pytest.mark.parametrize("n_tx,Nl", [(1, 1), (2, 2), (4, 4), (3, 2), (2, 1)])
def test_pdsch_mapping(emul, n_tx, Nl):
    L, m = emul
    rng = np.random.default_rng(900 + 10 * n_tx + Nl)
    segs, lay, stride = GPM.mixed_case(rng, n_tx, Nl)
    want = GPM.host_form(m, segs, lay, stride, n_tx)
    written = (want != CANARY).any(-1)
    assert written.sum() >= n_tx * sum(12 * s["rb_size"] for s in segs) - 8 and not written.all()
    lay0, arr = lay.copy(), m._pdm_seg_array(segs)
    grid_in_place(want, n_tx, stride, lambda tx: ok(L, L.slot_emul_pdsch_resource_mapping(lay.ctypes.data, tx, stride, n_tx, arr, len(segs))))
    assert np.array_equal(lay, lay0)


@pytest.mark.parametrize("n_tx,Nl,stride4", [(2, 1, False), (2, 2, True), (4, 2, False), (4, 4, True), (8, 3, False), (3, 2, True)])
def test_pdsch_mapping_precoded(emul, n_tx, Nl, stride4):
    L, m = emul
    rng = np.random.default_rng(1300 + 10 * n_tx + Nl)
    segs, prgs, pmis, lay, stride = GPP.mixed_precoded(rng, n_tx, Nl, stride4)
    table = GPP.table_for(rng, Nl)
    want = GPP.host_form(m, segs, prgs, pmis, table, lay, stride, n_tx)
    assert GPP.prg_edges_inside_groups(segs, prgs, pmis, stride, n_tx) > 0
    garr, keep, pmi_p, n_pmi, tab, n_pm = m._pre_args(segs, prgs, pmis, table)
    arr = m._pdm_seg_array(segs)
    grid_in_place(want, n_tx, stride, lambda tx: ok(L, L.slot_emul_pdsch_resource_mapping_precoded(lay.ctypes.data, tx, stride, n_tx, arr, garr, len(segs),
                                                                                                    pmi_p, n_pmi, tab, n_pm)))
    # all PMIs zero: the unit call's result
    zeros = [0] * len(pmis)
    garr, keep, pmi_p, n_pmi, tab, n_pm = m._pre_args(segs, prgs, zeros, None)
    unit = GPM.host_form(m, segs, lay, stride, n_tx)
    grid_in_place(unit, n_tx, stride, lambda tx: ok(L, L.slot_emul_pdsch_resource_mapping_precoded(lay.ctypes.data, tx, stride, n_tx, arr, garr, len(segs),
                                                                                                    pmi_p, n_pmi, tab, n_pm)))


# ---- the standalone QAM passes (tb_qam.hip): numpy is their host form (qam_np.py, layer_np.py) ------------------------------------
@pytest.mark.parametrize("Qm", [2, 4, 6, 8])
def test_modulation(emul, Qm):
    L, m = emul
    rng = np.random.default_rng(100 + Qm)
    for length in GQ.MOD_LENGTHS[Qm]:
        nw = (length + 31) // 32
        words = rng.integers(0, 1 << 32, nw + 1, dtype=np.uint64).astype(np.uint32)
        want = modulate_np(words, length, Qm)
        src = np.ascontiguousarray(words[:nw])
        for off in GQ.MOD_OFFS:                                          # 16-byte, 2-byte and 4-byte aligned outputs
            out = aligned16(2 * (length // Qm) + off + 8, np.int16, CANARY)
            ok(L, L.slot_emul_modulation(src.ctypes.data, length, Qm, out[off:].ctypes.data))
            assert np.array_equal(out[off:off + 2 * (length // Qm)].reshape(-1, 2), want), (Qm, length, off)
            assert (out[:off] == CANARY).all() and (out[off + 2 * (length // Qm):] == CANARY).all(), (Qm, length, off)


@pytest.mark.parametrize("Qm", [2, 4, 6, 8])
def test_ulsch_llr(emul, Qm):
    L, m = emul
    rng = np.random.default_rng(200 + Qm)
    for nb_re in GQ.LLR_NB_RE:
        y, mags = edge_symbols(rng, nb_re, Qm)
        want = demap_np(y, mags, Qm)
        for off in GQ.LLR_OFFS:                                          # 16-byte aligned planes and output / only 4-byte aligned ones
            planes = []
            for a in [y] + mags:
                t = aligned16(2 * nb_re + off, np.int16, 0)
                t[off:] = a.reshape(-1)
                planes.append(t[off:])
            ptrs = [p.ctypes.data for p in planes] + [None] * (4 - len(planes))
            out = aligned16(nb_re * Qm + off + 16, np.int16, CANARY)
            ok(L, L.slot_emul_ulsch_llr(*ptrs, nb_re, Qm, out[off:].ctypes.data))
            assert np.array_equal(out[off:off + nb_re * Qm], want), (Qm, nb_re, off)
            assert (out[:off] == CANARY).all() and (out[off + nb_re * Qm:] == CANARY).all(), (Qm, nb_re, off)


@pytest.mark.parametrize("Nl", [1, 2, 3, 4])
def test_layer_mapping(emul, Nl):
    L, m = emul
    rng = np.random.default_rng(500 + Nl)
    for per in GDS.LAYER_PER:
        n = per * Nl
        pts = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
        want = layer_map_np(pts, Nl)
        for stride in GDS.layer_strides(per):
            for off_in, off_out in GDS.LAYER_OFFS:                       # int16 offsets: 16-byte, 4-byte, 2-byte aligned arrays
                src = aligned16(2 * n + 8, np.int16, 0)
                src[off_in:off_in + 2 * n] = pts.reshape(-1)
                dst = aligned16(2 * Nl * stride + 8, np.int16, CANARY)
                ok(L, L.slot_emul_layer_mapping(src[off_in:].ctypes.data, n, Nl, dst[off_out:].ctypes.data, stride))
                assert (dst[:off_out] == CANARY).all()
                o = dst[off_out:off_out + 2 * Nl * stride].reshape(Nl, stride, 2)
                assert np.array_equal(o[:, :per], want), (Nl, per, stride, off_in, off_out)
                assert (o[:, per:] == CANARY).all() and (dst[off_out + 2 * Nl * stride:] == CANARY).all()


# ---- scrambling (tb_scrambling.hip, tb_scr_pack.hip, nr_scramble_map_tb_kernel): the bit-serial sequence is their host form.
# These kernels have a barrier, so every workgroup runs on 256 real threads: the sizes of test_gpu_scrambling.py up to two
# workgroups (32 * 1024 bits + 1), not its 245700 and 2^21 bits, which add workgroups and no branch ------------------------------
SCR_SIZES = [n for n in GS.SIZES if n <= 32 * 1024 + 1]


def test_scrambling(emul):
    L, m = emul
    rng = np.random.default_rng(2)
    assert SCR_SIZES == [1, 31, 32, 33, 1000, 32 * 1024 - 5, 32 * 1024, 32 * 1024 + 1]
    for i, n in enumerate(SCR_SIZES):
        p = GS.PARAMS[(i + 1) % len(GS.PARAMS)]
        for off in (0, 3):                                               # an input that is not 16-byte aligned takes the byte loads
            bits = rng.integers(0, 256, n, dtype=np.uint8)
            src = aligned16(n + off, np.uint8, 0)
            src[off:] = bits
            nw = (n + 31) // 32
            out = aligned16(nw + 8, np.uint32, 0xA5A5A5A5)
            ok(L, L.slot_emul_scramble_bits(src[off:].ctypes.data, n, c_init_of(*p), out.ctypes.data))
            assert np.array_equal(out[:nw], GS.scrambled_words(bits, *p)), (n, off, p)
            assert (out[nw:] == 0xA5A5A5A5).all()


def test_unscrambling(emul):
    L, m = emul
    rng = np.random.default_rng(4)
    for i, n in enumerate(SCR_SIZES):
        p = GS.PARAMS[(i + 2) % len(GS.PARAMS)]
        for off in (0, 1):
            llr = GS.special_llrs(rng, n + off + 40)
            t = aligned16(llr.size, np.int16, 0)
            t[:] = llr
            ok(L, L.slot_emul_unscramble_llr(t[off:].ctypes.data, n, c_init_of(*p)))
            ref = llr.copy()
            ref[off:off + n] = GS.unscrambled(llr[off:off + n], *p)
            assert np.array_equal(t, ref), (n, off, p)


class ScrJob(C.Structure):
    _fields_ = [("in_off", U64), ("out_off", U64), ("G", U32), ("c_init", U32)]


class SymJob(C.Structure):
    _fields_ = [("in_off", U64), ("out_off", U64), ("G", U32), ("c_init", U32), ("Qm", U32), ("Nl", U32)]


def test_scr_pack(emul):
    """three transport blocks in one launch: a partial last word, whole words, more than a workgroup's 1024 words; an input that is
    16-byte aligned and one that is not"""
    L, m = emul
    rng = np.random.default_rng(6)
    Gs, jobs, in_at, out_at = [33, 4096, 32 * 1024 + 7], (ScrJob * 3)(), 0, 4
    bits, want = [], []
    for i, G in enumerate(Gs):
        p = GS.PARAMS[i + 1]
        b = rng.integers(0, 256, G, dtype=np.uint8)
        in_at += i                                                       # 0, 1, 3 bytes off a 16-byte boundary
        jobs[i] = ScrJob(in_at, out_at, G, c_init_of(*p))
        bits.append((in_at, b))
        want.append((out_at // 4, GS.scrambled_words(b, *p)))
        in_at += (G + 15) // 16 * 16
        out_at += 4 * ((G + 31) // 32) + 8
    src = aligned16(in_at, np.uint8, 0)
    for at, b in bits:
        src[at:at + b.size] = b
    out = aligned16(out_at // 4, np.uint32, 0xA5A5A5A5)
    ref = out.copy()
    for at, w in want:
        ref[at:at + w.size] = w
    ok(L, L.slot_emul_scramble_bits_tb(jobs, 3, max(Gs), src.ctypes.data, out.ctypes.data))
    assert np.array_equal(out, ref), np.flatnonzero(out != ref)[:8]


def test_scramble_map_tb(emul):
    """the symbol encode's scrambling + mapping + layer mapping launch: every Qm, Nl 1..4, one block longer than a workgroup's
    4096 symbols"""
    L, m = emul
    rng = np.random.default_rng(7)
    shapes = [(2, 1, 2 * 5), (4, 2, 4 * 2 * 9), (6, 3, 6 * 3 * 11), (8, 4, 8 * 4 * 1030), (6, 2, 6 * 2 * 2049)]
    jobs, in_at, out_at = (SymJob * len(shapes))(), 0, 8
    bits, want = [], []
    for i, (Qm, Nl, G) in enumerate(shapes):
        p = GS.PARAMS[i % len(GS.PARAMS)]
        b = rng.integers(0, 256, G, dtype=np.uint8)
        jobs[i] = SymJob(in_at, out_at, G, c_init_of(*p), Qm, Nl)
        bits.append((in_at, b))
        planes = layer_map_np(modulate_np(GS.scrambled_words(b, *p), G, Qm), Nl)
        want.append((out_at // 2, planes.reshape(-1)))
        in_at += G + i
        out_at += 4 * (G // Qm) + 4 * (i + 1)
    src = aligned16(in_at, np.uint8, 0)
    for at, b in bits:
        src[at:at + b.size] = b
    out = aligned16(out_at // 2, np.int16, CANARY)
    ref = out.copy()
    for at, w in want:
        ref[at:at + w.size] = w
    ok(L, L.slot_emul_scramble_map_tb(jobs, len(shapes), max(G // Qm for Qm, Nl, G in shapes), src.ctypes.data, out.ctypes.data))
    assert np.array_equal(out, ref), np.flatnonzero(out != ref)[:8]
