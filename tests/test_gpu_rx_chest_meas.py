"""The measuring PUSCH channel estimation and the time average of its estimates on the GPU: the descriptor sets of
test_rx_chest_meas_host.py through DEVICE mem on a side stream, and HOST mem once.  ul_ch must equal pusch_channel_estimation's over
the whole array, max_ch / nvar the host form's (and the restatement's), the averaged array the restatement's over the whole array;
and one rank-2 slot each through the MMSE and the ML receiver runs estimation_meas -> level -> receiver -> decode on one stream
with no host value between rxdataF and the payload."""
import numpy as np
import pytest

import test_rx_chest_meas_host as H
import ul_slot_np as U

pytestmark = pytest.mark.gpu


def device_meas(m, b, reps=1, plain=False):
    """-> (ul_ch [ch_len, 2], max_ch, nvar) after `reps` calls on one set of arrays, on a side stream"""
    import torch
    n_tb = len(b["blocks"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rx_d = torch.from_numpy(b["rx"].reshape(-1).copy()).cuda()
        ch_d = torch.full((b["ch_len"] * 2,), H.FILL, dtype=torch.int16, device="cuda")
        dl_d = None if b["est_delay"] is None else torch.from_numpy(b["est_delay"].copy()).cuda()
        mx_d = torch.full((n_tb,), -1, dtype=torch.int32, device="cuda")
        nv_d = torch.full((n_tb,), -1, dtype=torch.int32, device="cuda")
        for _ in range(reps):
            if plain:
                m.pusch_channel_estimation(rx_d, b["rx_stride"], ch_d, b["ch_stride"], b["n_rx"], b["segs"], dl_d)
            else:
                m.pusch_channel_estimation_meas(rx_d, b["rx_stride"], ch_d, b["ch_stride"], b["n_rx"], b["segs"], b["seg_tb"], b["nvar_div"], dl_d, mx_d, nv_d)
    torch.cuda.synchronize()
    return ch_d.cpu().numpy().reshape(-1, 2), mx_d.cpu().numpy().tolist(), nv_d.cpu().numpy().view(np.uint32).tolist()


def host_form(m, b):
    """max_ch / nvar per block out of pusch_chest_meas_host per descriptor"""
    mx, nv = [0] * len(b["blocks"]), [0] * len(b["blocks"])
    for s, tb in zip(b["segs"], b["seg_tb"]):
        x, noise, nest = m.pusch_chest_meas_host(b["rx"], b["rx_stride"], b["n_rx"], s, b["est_delay"])
        mx[tb] = max(mx[tb], x)
        nv[tb] = (nv[tb] + (noise // nest if nest else 0)) & 0xffffffff
    return mx, [v // d for v, d in zip(nv, b["nvar_div"])]


@pytest.mark.parametrize("name", list(H.CASES))
def test_device_mode_equals_the_plain_call_and_the_host_form(hip, name):
    m = hip.ldpc
    b = H.build(name)
    want_ch = device_meas(m, b, plain=True)[0]
    want_mx, want_nv = host_form(m, b)
    ch, mx, nv = device_meas(m, b, reps=2)                               # the second call starts from accumulators of its own
    assert np.array_equal(ch, want_ch), (name, np.argwhere(ch != want_ch)[:4])
    assert mx == want_mx and nv == want_nv, (name, mx, want_mx, nv, want_nv)
    r_mx, r_nv, r_ch, _ = H.restated(name)
    assert mx == r_mx and nv == r_nv and np.array_equal(ch, r_ch), name


def test_host_mode_equals_device_mode(hip):
    m = hip.ldpc
    for name in ("three-blocks", "full-scale-t1i"):
        b = H.build(name)
        ch_d, mx_d, nv_d = device_meas(m, b)
        ch = np.full((b["ch_len"], 2), H.FILL, np.int16)
        _, mx, nv = m.pusch_channel_estimation_meas(b["rx"].reshape(-1, 2), b["rx_stride"], ch, b["ch_stride"], b["n_rx"], b["segs"], b["seg_tb"],
                                                    b["nvar_div"], b["est_delay"])
        assert np.array_equal(ch, ch_d) and mx.tolist() == mx_d and nv.tolist() == nv_d, name


def test_blocks_without_any_descriptor(hip):
    """DEVICE mem with blocks and no descriptor: the finishing launch alone writes 0 / 0"""
    m = hip.ldpc
    b = dict(H.build("small-m0-rb1"), segs=[], seg_tb=[], nvar_div=[3, 9], est_delay=None, blocks=[(1, 1), (1, 1)])
    ch, mx, nv = device_meas(m, b)
    assert mx == [0, 0] and nv == [0, 0] and bool((ch == H.FILL).all())


def test_time_average(hip):
    import torch
    m = hip.ldpc
    side = torch.cuda.Stream()
    for k, (n_sym, rb, shift, n_plane) in enumerate(H.AVG_CASES):
        ch, seg, stride = H.avg_case(n_sym, rb, shift, n_plane)
        want = H.avg_restated(ch, seg, stride, n_plane)
        with torch.cuda.stream(side):
            ch_d = torch.from_numpy(ch.reshape(-1).copy()).cuda()
            m.pusch_chest_time_avg(ch_d, stride, n_plane, [seg])
        side.synchronize()
        assert np.array_equal(ch_d.cpu().numpy().reshape(-1, 2), want), (n_sym, rb, shift)   # the whole array
        if k % 7 == 0:                                                   # HOST mem on a few
            assert np.array_equal(m.pusch_chest_time_avg(ch.copy(), stride, n_plane, [seg]), want), (n_sym, rb, shift)
    # two descriptors in one call, 22 and 300 PRBs (a second piece), both layers' planes
    rng = np.random.default_rng(5)
    ch = rng.integers(-32768, 32768, (40000, 2)).astype(np.int16)
    segs = [dict(ch_off=[3, 4003, 8003], n_sym=3, rb_size=22), dict(ch_off=[301, 4301, 8301, 12301], n_sym=4, rb_size=300)]
    want = ch
    for seg in segs:
        want = H.avg_restated(want, seg, 16390, 2)
    ch_d = torch.from_numpy(ch.reshape(-1).copy()).cuda()
    m.pusch_chest_time_avg(ch_d, 16390, 2, segs)
    torch.cuda.synchronize()
    assert np.array_equal(ch_d.cpu().numpy().reshape(-1, 2), want)


def test_device_refusals(hip):
    import torch
    m = hip.ldpc
    L = m._chest_meas_lib()
    b = H.build("three-blocks")
    rx_d = torch.from_numpy(b["rx"].reshape(-1).copy()).cuda()
    ch_d = torch.full((b["ch_len"] * 2,), H.FILL, dtype=torch.int16, device="cuda")
    mx_d, nv_d = torch.full((3,), -1, dtype=torch.int32, device="cuda"), torch.full((3,), -1, dtype=torch.int32, device="cuda")
    host = np.zeros(4, np.int32)
    segs, tb, div = m._chest_seg_array(b["segs"]), m._u32_array(b["seg_tb"]), m._u32_array(b["nvar_div"])

    def call(mx, nv, stream=None):
        return L.nrLDPC_hip_pusch_channel_estimation_meas(rx_d.data_ptr(), b["rx_stride"], ch_d.data_ptr(), b["ch_stride"], b["n_rx"], segs, len(b["segs"]),
                                                          None, tb, div, 3, mx, nv, m.MEM_DEVICE, stream)
    assert call(host.ctypes.data, nv_d.data_ptr()) < 0 and "DEVICE mem needs" in m.last_error()
    assert call(mx_d.data_ptr(), host.ctypes.data) < 0 and "DEVICE mem needs" in m.last_error()
    assert call(mx_d.data_ptr() + 2, nv_d.data_ptr()) < 0 and "DEVICE mem needs" in m.last_error()
    avg = m._chest_avg_seg_array([dict(ch_off=[0, 100], n_sym=2, rb_size=4)])
    assert L.nrLDPC_hip_pusch_chest_time_avg(np.zeros(400, np.int16).ctypes.data, 0, 1, avg, 1, m.MEM_DEVICE, None) < 0 and "DEVICE mem needs" in m.last_error()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    note = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        note.add_(1)
        rc = call(mx_d.data_ptr(), nv_d.data_ptr(), stream=side.cuda_stream)
        err = m.last_error()
        rc2 = L.nrLDPC_hip_pusch_chest_time_avg(ch_d.data_ptr(), 0, 1, avg, 1, m.MEM_DEVICE, side.cuda_stream)
        err2 = m.last_error()
    assert rc < 0 and "captured" in err and rc2 < 0 and "captured" in err2
    torch.cuda.synchronize()
    assert bool((ch_d == H.FILL).all()) and bool((mx_d == -1).all()) and bool((nv_d == -1).all()), "a refused call writes nothing"
    assert call(mx_d.data_ptr(), nv_d.data_ptr()) == 0
    torch.cuda.synchronize()
    assert mx_d.cpu().numpy().tolist() == H.restated("three-blocks")[0]


def run_slot(m, sl, seg_tb, nvar_div, record=None):
    """test_gpu_ul_slot.py's chain with pusch_channel_estimation_meas in front: max_ch and nvar never leave the device.  Returns
    numpy copies: ul_ch, max_ch, nvar, the shift, the record array, payload, ack, pass counts."""
    import torch
    c, tb = sl["case"], sl["tb"]
    n_rx = c["n_rx"]
    po, co, ho, nseg = m.tb_layout([tb])
    rxt = [dict(tb, round=0, llrLen=0)]
    harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
    out = torch.zeros(int(po[-1]) + 16, dtype=torch.uint8, device="cuda")
    ack = torch.zeros(1, dtype=torch.uint8, device="cuda")
    itm = torch.zeros(1, dtype=torch.int32, device="cuda")
    lv_d = torch.zeros(1, dtype=torch.int32, device="cuda")
    mc_d = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    nv_d = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    ch_d = torch.full((2 * n_rx * sl["ch_stride"] * 2,), U.FILL, dtype=torch.int16, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        if record is None:
            rx_d = torch.from_numpy(sl["rx"].reshape(-1).copy()).cuda()
            rec = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")
            m.pusch_channel_estimation_meas(rx_d, sl["rx_stride"], ch_d, sl["ch_stride"], n_rx, sl["csegs"], seg_tb, nvar_div,
                                            torch.from_numpy(sl["delay"].copy()).cuda(), mc_d, nv_d)
            if U.is_ml(c):
                m.ulsch_channel_level_grid_ml(ch_d, n_rx, sl["ch_stride"], sl["first"], mc_d, out=lv_d)
                m.ulsch_ml_2layers_grid(rx_d, ch_d, n_rx, sl["rx_stride"], sl["ch_stride"], sl["gsegs"], lv_d, rec)
            else:
                m.ulsch_channel_level_grid_mmse(ch_d, n_rx, sl["ch_stride"], sl["first"], mc_d, out=lv_d)
                m.ulsch_mmse_2layers_grid(rx_d, ch_d, n_rx, sl["rx_stride"], sl["ch_stride"], sl["gsegs"], lv_d, nv_d, rec)
        else:
            rec = torch.from_numpy(record).cuda()
        (m.ulsch_decode_scrambled_device if U.is_ml(c) else m.ulsch_decode_symbols_device)(rxt, rec, harq, out, ack, itm, [sl["scr"]])
    torch.cuda.synchronize()
    return (ch_d.cpu().numpy().reshape(-1, 2), int(mc_d[0]), int(nv_d.cpu().numpy().view(np.uint32)[0]), int(lv_d[0]), rec.cpu().numpy(),
            out.cpu().numpy()[:tb["A"] // 8], ack.cpu().numpy(), itm.cpu().numpy())


@pytest.mark.parametrize("name", H.E2E_SLOTS)
def test_rank2_slot_from_the_grid_to_the_payload_on_one_stream(hip, name):
    m = hip.ldpc
    sl, seg_tb, nvar_div, max_ch, nvar = H.slot_measured(name)
    tb = sl["tb"]
    ch_want = U.estimate_host(m, sl)
    lv_want, rec_tb = U.front_records(dict(sl, max_ch=max_ch, nvar=nvar), ch_want, None)   # the numpy receivers fed the restated values
    rec_want = np.zeros(int(m.tb_layout([tb])[1][-1]) + 16, np.int16)
    rec_want[:tb["G"]] = rec_tb
    ch, mc, nv, lv, rec, pay, ack, itm = run_slot(m, sl, seg_tb, nvar_div)
    assert np.array_equal(ch, ch_want) and (mc, nv) == (max_ch, nvar), (name, mc, max_ch, nv, nvar)
    assert lv == lv_want and np.array_equal(rec, rec_want), (name, lv, lv_want, np.flatnonzero(rec != rec_want)[:8])
    fed = run_slot(m, sl, seg_tb, nvar_div, record=rec_want)
    assert np.array_equal(pay, fed[5]) and np.array_equal(ack, fed[6]) and np.array_equal(itm, fed[7])
    assert ack.all() and np.array_equal(pay, sl["pay"]), (name, itm)
