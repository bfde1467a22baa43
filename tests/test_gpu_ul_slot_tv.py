"""The slots of ul_slot_tv_np.py -- several DMRS symbols, a channel that changes between them -- on the GPU, each chain on one side
stream with no host value between rxdataF and the payload.  One layer: pusch_channel_estimation with every DMRS symbol's
descriptors in one call, channel_level_grid, channel_compensation_grid, decode_symbols.  Two layers: pusch_channel_estimation_meas
with seg_tb naming the one block for all 2 n_dmrs descriptors and nvar_div = nr_of_symbols nrOfLayers n_rx, the _mmse or _ml level
and receiver, decode.  The grid descriptors are pusch_grid_segments' with alloc.dmrs_symbol = 255: ch_off differs from segment to
segment while the level is read at the first DMRS symbol.  ul_ch must equal the host form's over the whole array, max_ch / nvar,
the level and the record (the ML receiver's LLRs) the CPU chain's of test_ul_slot_tv_host.py bit for bit, the decoder's results
those of the same call fed that record, and the block must decode.  chest_time = 1: pusch_chest_time_avg between estimation and
level, the explicit first DMRS symbol in the descriptors.  test_ul_slot_tv_host.py shows on the CPU that any other descriptor
list fails these slots."""
import numpy as np
import pytest

import ul_slot_np as U
import ul_slot_tv_np as T

pytestmark = pytest.mark.gpu


def run_device(m, sl, gsegs, first, record=None, avg=None):
    """The chain on one side stream; record = None: from the grid; else the decode call alone on that record.  avg = the time
    average's descriptors (chest_time = 1) or None.  Returns numpy copies: ul_ch, max_ch, nvar (two layers; else None), the shift, the
    record array, payload, ack, pass counts."""
    import torch
    c, tb = sl["case"], sl["tb"]
    n_rx, L = c["n_rx"], c["n_layers"]
    po, co, ho, nseg = m.tb_layout([tb])
    rxt = [dict(tb, round=0, llrLen=0)]
    harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
    out = torch.zeros(int(po[-1]) + 16, dtype=torch.uint8, device="cuda")
    ack = torch.zeros(1, dtype=torch.uint8, device="cuda")
    itm = torch.zeros(1, dtype=torch.int32, device="cuda")
    lv_d = torch.zeros(1, dtype=torch.int32, device="cuda")
    mc_d = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    nv_d = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    ch_d = torch.full((L * n_rx * sl["ch_stride"] * 2,), U.FILL, dtype=torch.int16, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        if record is None:
            rx_d = torch.from_numpy(sl["rx"].reshape(-1).copy()).cuda()
            dl_d = torch.from_numpy(sl["delay"].copy()).cuda()
            rec = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")
            if L == 1:
                m.pusch_channel_estimation(rx_d, sl["rx_stride"], ch_d, sl["ch_stride"], n_rx, sl["csegs"], dl_d)
            else:
                m.pusch_channel_estimation_meas(rx_d, sl["rx_stride"], ch_d, sl["ch_stride"], n_rx, sl["csegs"], sl["seg_tb"], sl["nvar_div"], dl_d, mc_d, nv_d)
            if avg is not None:
                m.pusch_chest_time_avg(ch_d, sl["ch_stride"], L * n_rx, avg)
            if L == 1:
                m.ulsch_channel_level_grid(ch_d, n_rx, sl["ch_stride"], first, out=lv_d)
                m.ulsch_channel_compensation_grid(rx_d, ch_d, n_rx, sl["rx_stride"], sl["ch_stride"], gsegs, lv_d, rec)
            elif U.is_ml(c):                                               # rec holds the block's LLRs
                m.ulsch_channel_level_grid_ml(ch_d, n_rx, sl["ch_stride"], first, mc_d, out=lv_d)
                m.ulsch_ml_2layers_grid(rx_d, ch_d, n_rx, sl["rx_stride"], sl["ch_stride"], gsegs, lv_d, rec)
            else:
                m.ulsch_channel_level_grid_mmse(ch_d, n_rx, sl["ch_stride"], first, mc_d, out=lv_d)
                m.ulsch_mmse_2layers_grid(rx_d, ch_d, n_rx, sl["rx_stride"], sl["ch_stride"], gsegs, lv_d, nv_d, rec)
        else:
            rec = torch.from_numpy(record).cuda()
        (m.ulsch_decode_scrambled_device if U.is_ml(c) else m.ulsch_decode_symbols_device)(rxt, rec, harq, out, ack, itm, [sl["scr"]])
    torch.cuda.synchronize()
    two = L == 2 and record is None
    return (ch_d.cpu().numpy().reshape(-1, 2), int(mc_d[0]) if two else None, int(nv_d.cpu().numpy().view(np.uint32)[0]) if two else None, int(lv_d[0]),
            rec.cpu().numpy(), out.cpu().numpy()[:tb["A"] // 8], ack.cpu().numpy(), itm.cpu().numpy())


def check_chain(m, sl, ch_want, gsegs, first, avg=None):
    """the device chain against the CPU chain on ch_want (the estimates the receivers read) with the given descriptors"""
    c, tb, name = sl["case"], sl["tb"], sl["case"]["name"]
    want_meas = T.measured_host(m, sl) if c["n_layers"] == 2 else (None, None)
    slm = T.with_measured(m, sl)
    lv_want, rec_tb = U.front_records(dict(slm, gsegs=gsegs, first=first), ch_want, None)
    rec_want = np.zeros(int(m.tb_layout([tb])[1][-1]) + 16, np.int16)
    rec_want[:tb["G"]] = rec_tb
    ch, mc, nv, lv, rec, pay, ack, itm = run_device(m, sl, gsegs, first, avg=avg)
    # ul_ch over the whole array, fill included; the write set is 12 rb_size c16 per (descriptor, antenna)
    assert np.array_equal(ch, ch_want), (name, np.argwhere(ch != ch_want)[:4])
    per_plane = (ch != U.FILL).all(1).reshape(c["n_layers"] * c["n_rx"], -1).sum(1)
    assert per_plane.tolist() == [len(sl["dmrs"]) * 12 * c["rb"]] * (c["n_layers"] * c["n_rx"])
    assert (mc, nv) == want_meas, (name, mc, nv, want_meas)
    assert lv == lv_want and np.array_equal(rec, rec_want), (name, lv, lv_want, np.flatnonzero(rec != rec_want)[:8])
    fed = run_device(m, sl, gsegs, first, record=rec_want)
    assert np.array_equal(pay, fed[5]) and np.array_equal(ack, fed[6]) and np.array_equal(itm, fed[7])
    assert ack.all() and np.array_equal(pay, sl["pay"]), (name, itm)


@pytest.mark.parametrize("name", [c["name"] for c in T.CASES])
def test_changing_channel_slot_on_one_stream(hip, name):
    m = hip.ldpc
    sl = T.slot_of(m, name)
    tx = m.dlsch_encode_symbols_host([sl["tb"]], [sl["pay"]], [sl["scr"]])[0]
    assert np.array_equal(tx, sl["tx"]), "the slot's transmitter is dlsch_encode_symbols_host"
    assert len({g["ch_off"] for g in sl["gsegs"]}) == len(sl["dmrs"]) and sl["first"][0]["ch_off"] == min(g["ch_off"] for g in sl["gsegs"])
    check_chain(m, sl, U.estimate_host(m, sl), sl["gsegs"], sl["first"])


@pytest.mark.parametrize("name", [c["name"] for c in T.CASES_CT1])
def test_time_average_chain_on_one_stream(hip, name):
    m = hip.ldpc
    sl = T.slot_of(m, name)
    avg, gsegs, first, aseg = T.time_average_host(m, sl, U.estimate_host(m, sl))
    check_chain(m, sl, avg, gsegs, first, avg=[aseg])


def test_two_allocations_in_one_call(hip):
    """One estimation, one level and one compensation call for two allocations in one rxdataF / ul_ch array (two slots of the
    ring): block 0 with dmrs_symbol = 255 on DMRS symbols 2 and 11, block 1 with an explicit symbol on a slot with one DMRS symbol
    (3) and two CDM groups without data.  The level is per block, ch_off per segment: ul_ch equals the two host forms' at their
    places over the whole array and both records equal the blocks' own chains."""
    import torch
    m = hip.ldpc
    A, B = T.slot_of(m, "tv-1L-T1I"), U.slot_of(m, "1L-T1I-p2")
    n_rx, N = 2, 256
    assert A["case"]["n_rx"] == B["case"]["n_rx"] == n_rx and A["case"]["N"] == B["case"]["N"] == N
    assert A["alloc"]["dmrs_symbol"] == T.FOLLOW and B["alloc"]["dmrs_symbol"] == 3 and B["alloc"]["ul_dmrs_symb_pos"] == 1 << 3
    rec_off = (A["tb"]["G"] + 15) & ~15
    rx_stride, ch_stride = A["rx_stride"] + B["rx_stride"], A["ch_stride"] + B["ch_stride"]
    alloc_b = dict(B["alloc"], tb=1, rx_slot_off=B["alloc"]["rx_slot_off"] + A["rx_stride"], ch_off=B["alloc"]["ch_off"] + A["ch_stride"], rec_off=rec_off)
    gsegs, first = m.pusch_grid_segments([A["alloc"], alloc_b])
    assert gsegs[:len(A["gsegs"])] == A["gsegs"] and first[0] == A["first"][0] and len(gsegs) == len(A["gsegs"]) + len(B["gsegs"])
    csegs = A["csegs"] + [dict(s, rx_off=s["rx_off"] + A["rx_stride"], ch_off=s["ch_off"] + A["ch_stride"], delay_off=s["delay_off"] + len(A["csegs"]) * n_rx)
                          for s in B["csegs"]]
    rx = np.concatenate([A["rx"], B["rx"]], axis=1)
    want, ch_want = [], []
    for sl in (A, B):
        ch_sl = U.estimate_host(m, sl)
        want.append(U.front_records(sl, ch_sl, None))
        ch_want.append(ch_sl.reshape(n_rx, sl["ch_stride"], 2))
    ch_want = np.concatenate(ch_want, axis=1).reshape(-1, 2)              # each antenna: block 0's plane, then block 1's, fill included
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rx_d = torch.from_numpy(rx.reshape(-1).copy()).cuda()
        ch_d = torch.full((n_rx * ch_stride * 2,), U.FILL, dtype=torch.int16, device="cuda")
        lv_d = torch.zeros(2, dtype=torch.int32, device="cuda")
        rec = torch.zeros(rec_off + B["tb"]["G"] + 16, dtype=torch.int16, device="cuda")
        m.pusch_channel_estimation(rx_d, rx_stride, ch_d, ch_stride, n_rx, csegs, torch.from_numpy(np.concatenate([A["delay"], B["delay"]])).cuda())
        m.ulsch_channel_level_grid(ch_d, n_rx, ch_stride, first, out=lv_d)
        m.ulsch_channel_compensation_grid(rx_d, ch_d, n_rx, rx_stride, ch_stride, gsegs, lv_d, rec)
    torch.cuda.synchronize()
    rec = rec.cpu().numpy()
    assert np.array_equal(ch_d.cpu().numpy().reshape(-1, 2), ch_want)
    assert lv_d.cpu().numpy().tolist() == [want[0][0], want[1][0]]
    assert np.array_equal(rec[:A["tb"]["G"]], want[0][1]) and np.array_equal(rec[rec_off:rec_off + B["tb"]["G"]], want[1][1])
    assert not rec[A["tb"]["G"]:rec_off].any() and not rec[rec_off + B["tb"]["G"]:].any()


@pytest.mark.parametrize("name", ["tv-1L-T2I-3dmrs", "tv-2L-mmse"])
def test_host_mode_equals_device_mode(hip, name):
    m = hip.ldpc
    sl = T.slot_of(m, name)
    c = sl["case"]
    n_rx, L = c["n_rx"], c["n_layers"]
    ch_d, mc_d, nv_d, lv_d, rec_d = run_device(m, sl, sl["gsegs"], sl["first"])[:5]
    ch_h = np.full((L * n_rx * sl["ch_stride"], 2), U.FILL, np.int16)
    rx = sl["rx"].reshape(-1).copy()
    rec_h = np.zeros(rec_d.size, np.int16)
    if L == 1:
        m.pusch_channel_estimation(rx.reshape(-1, 2), sl["rx_stride"], ch_h, sl["ch_stride"], n_rx, sl["csegs"], sl["delay"].copy())
        lv_h = m.ulsch_channel_level_grid(ch_h.reshape(-1), n_rx, sl["ch_stride"], sl["first"])
        m.ulsch_channel_compensation_grid(rx, ch_h.reshape(-1), n_rx, sl["rx_stride"], sl["ch_stride"], sl["gsegs"], lv_h, rec_h)
    else:
        _, mc_h, nv_h = m.pusch_channel_estimation_meas(rx.reshape(-1, 2), sl["rx_stride"], ch_h, sl["ch_stride"], n_rx, sl["csegs"], sl["seg_tb"],
                                                        sl["nvar_div"], sl["delay"].copy())
        assert mc_h.tolist() == [mc_d] and nv_h.tolist() == [nv_d]
        lv_h = m.ulsch_channel_level_grid_mmse(ch_h.reshape(-1), n_rx, sl["ch_stride"], sl["first"], mc_h)
        m.ulsch_mmse_2layers_grid(rx, ch_h.reshape(-1), n_rx, sl["rx_stride"], sl["ch_stride"], sl["gsegs"], lv_h, nv_h.view(np.int32), rec_h)
    assert np.array_equal(ch_h, ch_d) and lv_h.tolist() == [lv_d] and np.array_equal(rec_h, rec_d)
