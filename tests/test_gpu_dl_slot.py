"""The DL transmit grid on the GPU against the float64 PDSCH model of dl_slot_np.py, on the cases test_dl_slot_host.py holds the CPU
forms to: payload bytes through dlsch_encode_symbols_device and pdsch_resource_mapping or pdsch_resource_mapping_precoded on one side
stream, only descriptors (and the PMIs and matrices) crossing the link.  The grid must equal the CPU forms' grid over the whole
array, canaries included, and, independently of that, lie within the model's derived bound.  Then the loop-back: the grid read as
the received one by pusch_channel_estimation (est_delay NULL), the level, compensation or the two-layer MMSE receiver and
ulsch_decode_symbols_device, for the ports, the DMRS type, the two-layer and the precoded cases the UL receiver can take; the payload
must come back exactly, with ACK.  test_dl_slot_host.py runs the same loop-backs on the CPU forms."""
import numpy as np
import pytest

import dl_slot_np as D
import test_dl_slot_host as H

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in D.CASES]


def payload_array(m, tb, pay):
    po = m.tb_layout([tb])[0]
    out = np.zeros(int(po[-1]) + 16, np.uint8)
    out[po[0]:po[0] + tb["A"] // 8] = pay
    return out


@pytest.mark.parametrize("name", NAMES)
def test_grid_on_one_stream_against_the_host_forms_and_the_model(hip, name):
    import torch
    m = hip.ldpc
    sl = H.slot_of(m, name)
    c, tb = sl["case"], sl["tb"]
    want = H.run_host(m, sl)
    co, total = m.tb_layout_symbols([tb])
    assert int(co[0]) == 0 and sl["alloc"]["lay_off"] == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pay_d = torch.from_numpy(payload_array(m, tb, sl["pay"])).cuda()
        lay_d = torch.zeros(total // 2 + 8, dtype=torch.int16, device="cuda")
        tx_d = torch.full(((c["n_tx"] + 1) * sl["stride"], 2), H.CANARY, dtype=torch.int16, device="cuda")
        m.dlsch_encode_symbols_device([tb], pay_d, lay_d, [sl["scr"]], stream=side.cuda_stream)
        if c["prg"] is None:
            m.pdsch_resource_mapping(lay_d, tx_d, sl["stride"], c["n_tx"], sl["segs"], stream=side.cuda_stream)
        else:
            m.pdsch_resource_mapping_precoded(lay_d, tx_d, sl["stride"], c["n_tx"], sl["segs"], sl["prgs"], c["pmis"], sl["table"], stream=side.cuda_stream)
    torch.cuda.synchronize()
    planes = lay_d.cpu().numpy()[:2 * c["Nl"] * sl["tx"].shape[1]].reshape(sl["tx"].shape)
    assert np.array_equal(planes, sl["tx"]), "the layer planes of the device call"
    got = tx_d.cpu().numpy().reshape(c["n_tx"] + 1, sl["stride"], 2)
    assert np.array_equal(got, want), (name, np.argwhere(got != want)[:4])
    e_max = H.check_grid(sl, got, "GPU")
    print(f"case {name}: GPU error {e_max:.3f} / bound {float(sl['bound'].max()):.3f}")


@pytest.mark.parametrize("key", sorted(H.LOOPS))
def test_loop_back_through_the_ul_receive_front(hip, key):
    import torch
    m = hip.ldpc
    lp = H.build_loop(m, key)
    c, tb = lp["case"], lp["tb"]
    L, n_ant, stride, ch_stride = c["n_layers"], c["n_rx"], lp["stride"], lp["ch_stride"]
    po, co, ho, _ = m.tb_layout([tb])
    total = m.tb_layout_symbols([tb])[1]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pay_d = torch.from_numpy(payload_array(m, tb, lp["pay"])).cuda()
        lay_d = torch.zeros(total // 2 + 8, dtype=torch.int16, device="cuda")
        grid = torch.zeros(2 * n_ant * stride, dtype=torch.int16, device="cuda")
        m.dlsch_encode_symbols_device([tb], pay_d, lay_d, [lp["scr"]], stream=side.cuda_stream)
        if lp["loop"]["precoded"]:
            m.pdsch_resource_mapping_precoded(lay_d, grid, stride, n_ant, lp["msegs"], lp["prgs"], lp["pmis"], lp["table"], stream=side.cuda_stream)
        else:
            m.pdsch_resource_mapping(lay_d, grid, stride, n_ant, lp["msegs"], stream=side.cuda_stream)
        ch_d = torch.zeros(2 * L * n_ant * ch_stride, dtype=torch.int16, device="cuda")
        harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
        out = torch.zeros(int(po[-1]) + 16, dtype=torch.uint8, device="cuda")
        ack = torch.zeros(1, dtype=torch.uint8, device="cuda")
        itm = torch.zeros(1, dtype=torch.int32, device="cuda")
        rec = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")
        lv_d = torch.zeros(1, dtype=torch.int32, device="cuda")
        m.pusch_channel_estimation(grid, stride, ch_d, ch_stride, n_ant, lp["csegs"], None)
        if L == 1:
            m.ulsch_channel_level_grid(ch_d, n_ant, ch_stride, lp["first"], out=lv_d)
            m.ulsch_channel_compensation_grid(grid, ch_d, n_ant, stride, ch_stride, lp["gsegs"], lv_d, rec)
        else:
            mc_d = torch.tensor([lp["max_ch"]], dtype=torch.int32, device="cuda")
            nv_d = torch.tensor([lp["nvar"]], dtype=torch.int32, device="cuda")
            m.ulsch_channel_level_grid_mmse(ch_d, n_ant, ch_stride, lp["first"], mc_d, out=lv_d)
            m.ulsch_mmse_2layers_grid(grid, ch_d, n_ant, stride, ch_stride, lp["gsegs"], lv_d, nv_d, rec)
        m.ulsch_decode_symbols_device([dict(tb, round=0, llrLen=0)], rec, harq, out, ack, itm, [lp["scr"]])
    torch.cuda.synchronize()
    assert ack.cpu().numpy().all(), (key, itm.cpu().numpy())
    assert np.array_equal(out.cpu().numpy()[:tb["A"] // 8], lp["pay"]), key
