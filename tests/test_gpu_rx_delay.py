"""The PUSCH delay search on the GPU (csrc/tb_rx_delay.hip) against the host form of the same header, on the cases of
test_rx_delay_host.py (all nine sizes in one call, rb_size 1 and 2, the full width at 1536, 275 PRBs at 4096, the peaks' positions,
n_rx 1, 2, 3 and 8 at delay_off = 2 + i (n_rx + 1), the ordered antennas in both modes, the ports, the wrap, averaging descriptors
and an all-zero symbol): delays and peaks bit for bit, nothing written but the write set.  HOST mem once, the refusals that need a
device, and the interpolating slots of ul_slot_np.py from rxdataF to the payload on one side stream with the search in front, so
that no delay comes from the host: the delays found are the channel's, ul_ch is the host form's given those, the block decodes."""
import numpy as np
import pytest

import rx_delay_np as D
import test_rx_delay_host as H
import ul_slot_np as U

pytestmark = pytest.mark.gpu


def device_search(m, b, flags, peak=True, reps=1):
    import torch
    rx_d = torch.from_numpy(b["rx"].reshape(-1).copy()).cuda()
    d_d = torch.full((b["n_res"],), H.FILL_D, dtype=torch.int32, device="cuda")
    p_d = torch.full((b["n_res"],), H.FILL_P, dtype=torch.float32, device="cuda") if peak else None
    for _ in range(reps):
        m.pusch_est_delay(rx_d, b["rx_stride"], b["n_rx"], b["segs"], flags, d_d, p_d)
    torch.cuda.synchronize()
    return d_d.cpu().numpy(), p_d.cpu().numpy() if peak else None


@pytest.mark.parametrize("name", list(H.CASES))
def test_device_mode_equals_the_host_form(hip, name):
    m = hip.ldpc
    b = H.build(name)
    for flags in H.FLAGS:
        want_d, want_p = H.host_form(m, b, flags)
        d, p = device_search(m, b, flags, reps=2 if name == "ports" else 1)
        assert np.array_equal(d, want_d), (name, flags, d, want_d)
        assert np.array_equal(p.view(np.uint32), want_p.view(np.uint32)), (name, flags, p, want_p)
    d, _ = device_search(m, b, D.RUNNING_MAX, peak=False)
    assert np.array_equal(d, H.host_form(m, b, D.RUNNING_MAX)[0])


def test_host_mode_equals_the_host_form(hip):
    m = hip.ldpc
    b = H.build("nine-sizes")
    for flags in H.FLAGS:
        want_d, want_p = H.host_form(m, b, flags)
        d, p = m.pusch_est_delay(b["rx"].reshape(-1, 2), b["rx_stride"], b["n_rx"], b["segs"], flags)
        for s in b["segs"]:
            o = slice(s["delay_off"], s["delay_off"] + b["n_rx"])
            assert np.array_equal(d[o], want_d[o]) and np.array_equal(p[o].view(np.uint32), want_p[o].view(np.uint32)), (flags, s["fft_size"])


def test_averaging_descriptors_alone(hip):
    """no search launch at all: the combining launch writes 0 and 0"""
    m = hip.ldpc
    b = H.build("ports")
    b = dict(b, segs=[dict(s, mode=2 + (s["mode"] & 1)) for s in b["segs"][:2]])
    d, p = device_search(m, b, D.RUNNING_MAX)
    for s in b["segs"]:
        o = slice(s["delay_off"], s["delay_off"] + b["n_rx"])
        assert not d[o].any() and not p[o].any()
        d[o], p[o] = H.FILL_D, H.FILL_P
    assert (d == H.FILL_D).all() and (p == H.FILL_P).all()


def test_device_refusals(hip):
    import torch
    m = hip.ldpc
    L = m._delay_lib()
    b = H.build("ports")
    rx_d = torch.from_numpy(b["rx"].reshape(-1).copy()).cuda()
    d_d = torch.full((b["n_res"],), H.FILL_D, dtype=torch.int32, device="cuda")
    p_d = torch.full((b["n_res"],), H.FILL_P, dtype=torch.float32, device="cuda")
    host = np.zeros(b["n_res"], np.int32)
    segs = m._chest_seg_array(b["segs"])

    def call(rx, d, p, stream=None, flags=0):
        return L.nrLDPC_hip_pusch_est_delay(rx, b["rx_stride"], b["n_rx"], segs, len(b["segs"]), flags, d, p, m.MEM_DEVICE, stream)
    assert call(rx_d.data_ptr(), host.ctypes.data, p_d.data_ptr()) < 0 and "DEVICE mem needs" in m.last_error()
    assert call(rx_d.data_ptr(), d_d.data_ptr(), host.ctypes.data) < 0 and "DEVICE mem needs" in m.last_error()
    assert call(b["rx"].ctypes.data, d_d.data_ptr(), p_d.data_ptr()) < 0 and "DEVICE mem needs" in m.last_error()
    assert call(rx_d.data_ptr(), d_d.data_ptr() + 2, p_d.data_ptr()) < 0 and "DEVICE mem needs" in m.last_error()
    assert call(rx_d.data_ptr() + 2, d_d.data_ptr(), p_d.data_ptr()) < 0 and "DEVICE mem needs" in m.last_error()
    assert call(rx_d.data_ptr(), None, p_d.data_ptr()) < 0 and "null argument" in m.last_error()
    assert call(rx_d.data_ptr(), d_d.data_ptr(), p_d.data_ptr(), flags=2) < 0 and "flags must be" in m.last_error()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    note = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        note.add_(1)
        rc = call(rx_d.data_ptr(), d_d.data_ptr(), p_d.data_ptr(), stream=side.cuda_stream)
        err = m.last_error()
    assert rc < 0 and "captured" in err
    torch.cuda.synchronize()
    assert bool((d_d == H.FILL_D).all()) and bool((p_d == H.FILL_P).all()), "a refused call writes nothing"
    assert call(rx_d.data_ptr(), d_d.data_ptr(), p_d.data_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_d.cpu().numpy(), H.host_form(m, b, 0)[0])


# ---------------------------------------------------------------------------------------------------------
# from rxdataF to the payload with no delay from the host
# ---------------------------------------------------------------------------------------------------------
def run_slot(m, sl, meas, record=None):
    """test_gpu_ul_slot.py's chain (meas: test_gpu_rx_chest_meas.py's, max_ch and nvar from the estimation call) with pusch_est_delay
    in PER_ANTENNA mode in front.  Without meas the two-layer receivers' max_ch and nvar are the slot's known values, uploaded as
    test_gpu_ul_slot.py uploads them.  Returns numpy copies: the delays, ul_ch, the shift, the record, payload, ack, pass counts."""
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
    mc_d = torch.tensor([-1 if meas else sl["max_ch"]], dtype=torch.int32, device="cuda")
    nv_d = torch.tensor([-1 if meas else sl["nvar"]], dtype=torch.int32, device="cuda")
    dl_d = torch.full((sl["delay"].size,), H.FILL_D, dtype=torch.int32, device="cuda")
    ch_d = torch.full((L * n_rx * sl["ch_stride"] * 2,), U.FILL, dtype=torch.int16, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        if record is None:
            rx_d = torch.from_numpy(sl["rx"].reshape(-1).copy()).cuda()
            rec = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")
            m.pusch_est_delay(rx_d, sl["rx_stride"], n_rx, sl["csegs"], D.PER_ANTENNA, dl_d)
            if meas:
                a = sl["alloc"]
                m.pusch_channel_estimation_meas(rx_d, sl["rx_stride"], ch_d, sl["ch_stride"], n_rx, sl["csegs"], [0] * len(sl["csegs"]),
                                                [a["nr_of_symbols"] * L * n_rx], dl_d, mc_d, nv_d)
            else:
                m.pusch_channel_estimation(rx_d, sl["rx_stride"], ch_d, sl["ch_stride"], n_rx, sl["csegs"], dl_d)
            if L == 1:
                m.ulsch_channel_level_grid(ch_d, n_rx, sl["ch_stride"], sl["first"], out=lv_d)
                m.ulsch_channel_compensation_grid(rx_d, ch_d, n_rx, sl["rx_stride"], sl["ch_stride"], sl["gsegs"], lv_d, rec)
            elif U.is_ml(c):
                m.ulsch_channel_level_grid_ml(ch_d, n_rx, sl["ch_stride"], sl["first"], mc_d, out=lv_d)
                m.ulsch_ml_2layers_grid(rx_d, ch_d, n_rx, sl["rx_stride"], sl["ch_stride"], sl["gsegs"], lv_d, rec)
            else:
                m.ulsch_channel_level_grid_mmse(ch_d, n_rx, sl["ch_stride"], sl["first"], mc_d, out=lv_d)
                m.ulsch_mmse_2layers_grid(rx_d, ch_d, n_rx, sl["rx_stride"], sl["ch_stride"], sl["gsegs"], lv_d, nv_d, rec)
        else:
            rec = torch.from_numpy(record).cuda()
        (m.ulsch_decode_scrambled_device if U.is_ml(c) else m.ulsch_decode_symbols_device)(rxt, rec, harq, out, ack, itm, [sl["scr"]])
    torch.cuda.synchronize()
    return (dl_d.cpu().numpy(), ch_d.cpu().numpy().reshape(-1, 2), int(lv_d[0]), rec.cpu().numpy(), out.cpu().numpy()[:tb["A"] // 8], ack.cpu().numpy(),
            itm.cpu().numpy())


@pytest.mark.parametrize("name", H.SLOTS)
def test_slot_from_the_grid_to_the_payload_with_no_delay_from_the_host(hip, name):
    import test_rx_chest_meas_host as MH
    m = hip.ldpc
    meas = name in MH.E2E_SLOTS                                          # the two-layer slots that decode with the measured nvar (see there)
    sl = MH.slot_measured(name)[0] if meas else U.slot_of(m, name)
    tb = sl["tb"]
    ch_want = U.estimate_host(m, sl)                                     # the host form given tau[a]
    known = dict(sl, max_ch=MH.slot_measured(name)[3], nvar=MH.slot_measured(name)[4]) if meas else sl
    lv_want, rec_tb = U.front_records(known, ch_want, None)
    rec_want = np.zeros(int(m.tb_layout([tb])[1][-1]) + 16, np.int16)
    rec_want[:tb["G"]] = rec_tb
    dl, ch, lv, rec, pay, ack, itm = run_slot(m, sl, meas)
    assert np.array_equal(dl, sl["delay"]), (name, dl, sl["delay"])      # the delays found are tau[a]
    assert np.array_equal(ch, ch_want), (name, np.argwhere(ch != ch_want)[:4])
    assert lv == lv_want and np.array_equal(rec, rec_want), (name, lv, lv_want, np.flatnonzero(rec != rec_want)[:8])
    fed = run_slot(m, sl, meas, record=rec_want)
    assert np.array_equal(pay, fed[4]) and np.array_equal(ack, fed[5]) and np.array_equal(itm, fed[6])
    assert ack.all() and np.array_equal(pay, sl["pay"]), (name, itm)
