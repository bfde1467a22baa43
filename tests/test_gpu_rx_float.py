"""The three UL receivers on the GPU against float64 detectors (rx_float_np.py): the cases of test_rx_float_host.py -- coupled
layers at correlation 0, 0.5, 0.8 and 0.95, two noise levels -- laid out on a 256-point OFDM grid and run through
channel_level_grid -> channel_compensation_grid -> ulsch_llr (one layer), channel_level_grid_mmse -> mmse_2layers_grid -> ulsch_llr
and channel_level_grid_ml -> ml_2layers_grid, in device mode with the level's output as the receiver's shift.  Every LLR of every
RE must lie within the bound (rx_float_np.BOUNDS) of the model and equal the numpy restatement of the reference.

One block per run (case, nvar), four segments each in an OFDM symbol of its own: 6 and 18 REs (DMRS1, 1 and 3 RBs: a partial last
group), 36 REs (FULL) and the measurement symbol of 240 REs (FULL) that the grid's wrap cuts inside a thread's group of four."""
import numpy as np
import pytest

import rx_float_np as F
from test_gpu_rx_grid import p_of
from test_rx_float_host import bound_of, model_llrs, restated

pytestmark = pytest.mark.gpu
N = 256
FULL, DMRS1 = 0, 1
PATTERNS = (DMRS1, DMRS1, FULL, FULL)             # of F.SEGMENTS
WRAP_AT = 101                                     # the measurement symbol's first RE behind the wrap: inside a group
FILL_RX, FILL_CH = 1234, -4321


def lay_out(receiver, runs, n_rx):
    """The runs' segments on the grid.  Returns (segs, first, rx, ch, rx_stride, ch_stride, rec_off per block, record length)."""
    L = 1 if receiver == "single" else 2
    S = sum(F.SEGMENTS)
    n_sym = len(F.SEGMENTS) * len(runs)
    rx_stride, ch_stride = n_sym * N + 5, n_sym * N + 9
    rx = np.full((n_rx, rx_stride, 2), FILL_RX, np.int16)
    ch = np.full((L * n_rx, ch_stride, 2), FILL_CH, np.int16)
    segs, first, rec_offs, rec_at, k = [], [], [], 2, 0
    for tb, (cs, extra, lv, want) in enumerate(runs):
        Qm = cs["Qm"]
        rec_offs.append(rec_at)
        for (at, nb), pattern in zip(F.segments_of(cs), PATTERNS):
            start_re = N - p_of(pattern, WRAP_AT) if nb == F.SEGMENTS[-1] else 7 + 12 * (k % 5)
            s = dict(tb=tb, Qm=Qm, pattern=pattern, nb_re=nb, plane=L * S, sym_off=at, fft_size=N, start_re=start_re, rx_off=k * N + 2, ch_off=k * N + 3,
                     rec_off=rec_at)
            idx = np.array([p_of(pattern, j) for j in range(nb)])
            assert idx[-1] < N and (nb != F.SEGMENTS[-1] or start_re + idx[-1] >= N)
            rx[:, s["rx_off"] + (start_re + idx) % N] = (cs["rx1"] if receiver == "single" else cs["rx"])[:, at:at + nb]
            ch[:, s["ch_off"] + idx] = (cs["ch"][0] if receiver == "single" else cs["ch"].reshape(2 * n_rx, -1, 2))[:, at:at + nb]
            segs.append(s)
            k += 1
        first.append(segs[-1])
        rec_at += Qm * L * S + 2 * (tb % 3)                                # a record or an LLR range of G = Qm L S int16
    return segs, first, rx, ch, rx_stride, ch_stride, rec_offs, rec_at + 16


def run_receiver(m, receiver, n_rx):
    """(runs, levels, LLRs per run) out of the GPU calls on one side stream"""
    import torch
    runs = [r for r in restated(receiver).values() if r[0]["n_rx"] == n_rx]
    assert len({(r[0]["Qm"], r[0]["c"]) for r in runs}) == len({r[0]["Qm"] for r in runs}) * (1 if receiver == "single" else len(F.CORRELATIONS))
    segs, first, rx, ch, rx_stride, ch_stride, rec_offs, rec_len = lay_out(receiver, runs, n_rx)
    S, L = sum(F.SEGMENTS), 1 if receiver == "single" else 2
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    outs = []
    with torch.cuda.stream(side):
        rx_d, ch_d = torch.from_numpy(rx.reshape(-1)).cuda(), torch.from_numpy(ch.reshape(-1)).cuda()
        rec = torch.zeros(rec_len, dtype=torch.int16, device="cuda")
        lv_d = torch.full((len(runs),), -1, dtype=torch.int32, device="cuda")
        mc_d = torch.tensor([r[0]["max_ch"] for r in runs], dtype=torch.int32, device="cuda")
        if receiver == "single":
            m.ulsch_channel_level_grid(ch_d, n_rx, ch_stride, first, out=lv_d)
            m.ulsch_channel_compensation_grid(rx_d, ch_d, n_rx, rx_stride, ch_stride, segs, lv_d, rec)
        elif receiver == "mmse":
            nv_d = torch.tensor([r[1][0] for r in runs], dtype=torch.int32, device="cuda")
            m.ulsch_channel_level_grid_mmse(ch_d, n_rx, ch_stride, first, mc_d, out=lv_d)
            m.ulsch_mmse_2layers_grid(rx_d, ch_d, n_rx, rx_stride, ch_stride, segs, lv_d, nv_d, rec)
        else:
            m.ulsch_channel_level_grid_ml(ch_d, n_rx, ch_stride, first, mc_d, out=lv_d)
            m.ulsch_ml_2layers_grid(rx_d, ch_d, n_rx, rx_stride, ch_stride, segs, lv_d, rec)
        for (cs, extra, lv, want), o in zip(runs, rec_offs):
            Qm, plane = cs["Qm"], L * S
            if receiver == "ml":
                outs.append(rec[o:o + Qm * plane])
            else:                                                          # the record's planes through the demapper
                llr = torch.zeros(Qm * plane, dtype=torch.int16, device="cuda")
                pl = [rec[o + 2 * k * plane:o + 2 * (k + 1) * plane] for k in range(Qm // 2)]
                m.ulsch_llr(pl[0], pl[1:], Qm, out=llr)
                outs.append(llr)
    torch.cuda.synchronize()
    shape = (S, -1) if receiver == "single" else (S, 2, -1)
    return runs, lv_d.cpu().numpy().tolist(), [o.cpu().numpy().astype(np.int64).reshape(shape) for o in outs]


@pytest.mark.parametrize("receiver,n_rx", [("single", 2), ("single", 4), ("single", 3), ("mmse", 2), ("mmse", 4), ("ml", 2), ("ml", 4), ("ml", 3)])
def test_grid_receivers_within_the_bound_of_the_float_model(hip, receiver, n_rx):
    runs, levels, llrs = run_receiver(hip.ldpc, receiver, n_rx)
    assert len(runs) >= 8 and levels == [r[2] for r in runs]
    worst = {}
    for (cs, extra, lv, want), got in zip(runs, llrs):
        assert got.shape == want.shape
        d = float(np.abs(got - model_llrs(receiver, cs, lv, extra)).max())
        worst[cs["Qm"]] = max(worst.get(cs["Qm"], 0.0), d)
        assert d <= bound_of(receiver, cs), (cs["name"], extra, d)
        assert np.array_equal(got, want), (cs["name"], extra, np.argwhere(got != want)[:4])
    print(receiver, n_rx, {Qm: f"{d:.2f} of {F.BOUNDS[(receiver, Qm)][1]}" for Qm, d in worst.items()})
