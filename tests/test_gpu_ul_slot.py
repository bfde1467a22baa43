"""The UL receive chain on the GPU on the frequency-selective slots of ul_slot_np.py, every DMRS port on the air: one
pusch_channel_estimation call for the descriptors of every layer (layer l's set at ch_off + l n_rx ch_stride), channel_level_grid
and channel_compensation_grid (one layer) or channel_level_grid_mmse and mmse_2layers_grid (two layers), and decode_symbols -- two
layers below 64QAM: channel_level_grid_ml, ml_2layers_grid and decode_scrambled on the LLRs --, all on one side stream with nothing
but descriptors, est_delay, max_ch and nvar uploaded.  ul_ch must equal the CPU form's estimates over the whole array, the shifts and records the numpy receivers run on those estimates, the decoder's results those of the same call
fed the numpy record; and the block must decode.  test_ul_slot_host.py holds the same estimates to the true channel and shows on
the CPU that a subtly wrong estimator would fail these slots."""
import numpy as np
import pytest

import ul_slot_np as U

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in U.CASES]
TWO_LAYER = [c["name"] for c in U.CASES if c["n_layers"] == 2]


def run_device(m, sl, record=None):
    """The chain on one side stream; record = None: from the grid; else decode_symbols alone on that record.  Returns numpy copies:
    ul_ch (None with a record), the shift, the record array, payload bytes, ack, pass counts, soft buffers."""
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
    ch_d = None
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        if record is None:
            rx_d = torch.from_numpy(sl["rx"].reshape(-1).copy()).cuda()
            ch_d = torch.full((L * n_rx * sl["ch_stride"] * 2,), U.FILL, dtype=torch.int16, device="cuda")
            rec = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")
            m.pusch_channel_estimation(rx_d, sl["rx_stride"], ch_d, sl["ch_stride"], n_rx, sl["csegs"], torch.from_numpy(sl["delay"].copy()).cuda())
            if L == 1:
                m.ulsch_channel_level_grid(ch_d, n_rx, sl["ch_stride"], sl["first"], out=lv_d)
                m.ulsch_channel_compensation_grid(rx_d, ch_d, n_rx, sl["rx_stride"], sl["ch_stride"], sl["gsegs"], lv_d, rec)
            elif U.is_ml(c):                                               # rec holds the block's LLRs
                mc_d = torch.tensor([sl["max_ch"]], dtype=torch.int32, device="cuda")
                m.ulsch_channel_level_grid_ml(ch_d, n_rx, sl["ch_stride"], sl["first"], mc_d, out=lv_d)
                m.ulsch_ml_2layers_grid(rx_d, ch_d, n_rx, sl["rx_stride"], sl["ch_stride"], sl["gsegs"], lv_d, rec)
            else:
                mc_d = torch.tensor([sl["max_ch"]], dtype=torch.int32, device="cuda")
                nv_d = torch.tensor([sl["nvar"]], dtype=torch.int32, device="cuda")
                m.ulsch_channel_level_grid_mmse(ch_d, n_rx, sl["ch_stride"], sl["first"], mc_d, out=lv_d)
                m.ulsch_mmse_2layers_grid(rx_d, ch_d, n_rx, sl["rx_stride"], sl["ch_stride"], sl["gsegs"], lv_d, nv_d, rec)
        else:
            rec = torch.from_numpy(record).cuda()
        (m.ulsch_decode_scrambled_device if U.is_ml(c) else m.ulsch_decode_symbols_device)(rxt, rec, harq, out, ack, itm, [sl["scr"]])
    torch.cuda.synchronize()
    return (None if ch_d is None else ch_d.cpu().numpy().reshape(-1, 2), int(lv_d[0]), rec.cpu().numpy(), out.cpu().numpy()[:tb["A"] // 8],
            ack.cpu().numpy(), itm.cpu().numpy(), harq.cpu().numpy())


@pytest.mark.parametrize("name", NAMES)
def test_selective_slot_on_one_stream(hip, name):
    m = hip.ldpc
    sl = U.slot_of(m, name)
    c, tb = sl["case"], sl["tb"]
    tx = m.dlsch_encode_symbols_host([tb], [sl["pay"]], [sl["scr"]])[0]
    assert np.array_equal(tx, sl["tx"]), "the slot's transmitter is dlsch_encode_symbols_host"
    # the CPU side: the host form's estimates and the numpy receivers on them
    ch_want = U.estimate_host(m, sl)
    lv_want, rec_tb = U.front_records(sl, ch_want, None)
    co = m.tb_layout([tb])[1]
    rec_want = np.zeros(int(co[-1]) + 16, np.int16)
    rec_want[:tb["G"]] = rec_tb
    ch, lv, rec, pay, ack, itm, harq = run_device(m, sl)
    # ul_ch over the whole array, fill included; the write set is 12 rb_size c16 per (descriptor, antenna)
    assert np.array_equal(ch, ch_want), (name, np.argwhere(ch != ch_want)[:4])
    per_plane = (ch != U.FILL).all(1).reshape(c["n_layers"] * c["n_rx"], -1).sum(1)
    assert per_plane.tolist() == [12 * c["rb"]] * (c["n_layers"] * c["n_rx"])
    at = sl["csegs"][0]["ch_off"]
    assert (U.planes_of(sl, ch) != U.FILL).all() and at > 0
    assert lv == lv_want and np.array_equal(rec, rec_want), (name, lv, lv_want, np.flatnonzero(rec != rec_want)[:8])
    # the decoder on the numpy record gives the same payload, ACK, pass counts and soft buffers
    fed = run_device(m, sl, record=rec_want)
    for a, b in zip((pay, ack, itm, harq), fed[3:]):
        assert np.array_equal(a, b)
    assert ack.all() and np.array_equal(pay, sl["pay"]), (name, itm)


def test_host_mode_equals_device_mode(hip):
    """HOST mode of the estimation call (both layers' descriptors in one call) and of the MMSE calls on one two-layer slot"""
    m = hip.ldpc
    sl = U.slot_of(m, TWO_LAYER[0])
    c, tb = sl["case"], sl["tb"]
    n_rx = c["n_rx"]
    ch_d, lv_d, rec_d = run_device(m, sl)[:3]
    ch_h = np.full((2 * n_rx * sl["ch_stride"], 2), U.FILL, np.int16)
    rx = sl["rx"].reshape(-1).copy()
    m.pusch_channel_estimation(rx.reshape(-1, 2), sl["rx_stride"], ch_h, sl["ch_stride"], n_rx, sl["csegs"], sl["delay"].copy())
    assert np.array_equal(ch_h, ch_d)
    lv_h = m.ulsch_channel_level_grid_mmse(ch_h.reshape(-1), n_rx, sl["ch_stride"], sl["first"], np.array([sl["max_ch"]], np.int32))
    assert lv_h.tolist() == [lv_d]
    rec_h = np.zeros(rec_d.size, np.int16)
    m.ulsch_mmse_2layers_grid(rx, ch_h.reshape(-1), n_rx, sl["rx_stride"], sl["ch_stride"], sl["gsegs"], lv_h, np.array([sl["nvar"]], np.int32), rec_h)
    assert np.array_equal(rec_h, rec_d)
