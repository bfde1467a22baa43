"""The six slot-level calls that upload descriptor tables -- pusch_channel_estimation, ulsch_channel_level_grid,
ulsch_channel_compensation_grid, ulsch_channel_level, ulsch_channel_compensation and pdsch_resource_mapping -- back to back on one
thread, each with numpy arrays (HOST mem: the thread's staging buffers) and with torch tensors on a non-default stream (DEVICE mem:
the thread's page-locked descriptor area), so that every call finds the contexts as the call before it left them.  A small slot, then
a large one whose staged inputs outgrow the small one's buffers, then the small one again in the buffers the large one left.  Every
output is compared for equality with the CPU forms (pusch_chest_host, ulsch_extract_host + ulsch_level_host / ulsch_compensate_host,
pdsch_map_host) on canary-filled arrays."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = 0x5a5a
N_ANT, QM, DMRS_SYM = 2, 4, 2                                          # n_rx = n_tx = 2, 16QAM, one type-1 DMRS symbol
_cases = {}


def slot_case(m, N, rb):
    """One PUSCH and one PDSCH allocation of rb PRBs over 14 symbols whose last PRB wraps round the end of an N-point grid (start_re
    = N - 12, 116 for N = 128).  The records start at c16 phase 1 (rec_off 2), the estimates at phase 3 (ch_off 7), the received
    and the transmit grid at phase 3 and 1 (slot offsets 3 and 1), the layer planes at phase 3.  The inputs and what the CPU forms
    make of them, computed once per shape."""
    if (N, rb) in _cases:
        return _cases[(N, rb)]
    rng = np.random.default_rng(N + rb)
    S = (13 * 12 + 6) * rb                                             # data REs: 13 full symbols and the odd subcarriers of the DMRS symbol
    ul = dict(tb=0, Qm=QM, dmrs_config_type=0, num_dmrs_cdm_grps_no_data=1, dmrs_symbol=DMRS_SYM, fft_size=N, first_carrier_offset=N - 12,
              bwp_start=0, rb_start=0, rb_size=rb, start_symbol=0, nr_of_symbols=14, ul_dmrs_symb_pos=1 << DMRS_SYM, plane=S, rx_slot_off=3,
              ch_off=7, rec_off=2)
    dl = dict(Nl=2, plane=S, dmrs_config_type=0, num_dmrs_cdm_grps_no_data=1, dmrs_ports=0b11, scid=1, dl_dmrs_scrambling_id=99, slot=4, si_rnti=0,
              amp=512, fft_size=N, first_carrier_offset=N - 12, bwp_start=0, rb_start=0, rb_size=rb, start_symbol=0, nr_of_symbols=14,
              dl_dmrs_symb_pos=1 << DMRS_SYM, tx_slot_off=1, lay_off=6)
    c = dict(N=N, rb=rb, S=S)
    c["gsegs"], c["first"] = m.pusch_grid_segments([ul])
    c["csegs"] = m.pusch_chest_segments([ul], [dict(slot=4, scid=1, dmrs_scrambling_id=99, port=0, chest_freq=0)], N_ANT)
    c["msegs"] = m.pdsch_map_segments([dl])
    assert len(c["gsegs"]) == 14 and len(c["csegs"]) == 1 and len(c["msegs"]) == 14
    assert c["gsegs"][0]["start_re"] == N - 12 and c["gsegs"][0]["start_re"] + 12 * rb > N
    rs, cs, ts = c["rs"], c["cs"], c["ts"] = 14 * N + 3 + 5, 14 * N + 7 + 6, 14 * N + 1 + 4
    rx = c["rx"] = rng.integers(-3000, 3000, (N_ANT * rs, 2)).astype(np.int16)
    c["delay"] = np.array([3, -2], np.int32)
    lay = c["lay"] = rng.integers(-32768, 32768, (3 + 2 * S + 4, 2)).astype(np.int16)
    # channel estimation: one descriptor, antenna by antenna
    ch = np.full((N_ANT * cs, 2), CANARY, np.int16)
    for s in c["csegs"]:
        for a in range(N_ANT):
            m.pusch_chest_host(rx, dict(s, rx_off=s["rx_off"] + a * rs, ch_off=s["ch_off"] + a * cs), int(c["delay"][s["delay_off"] + a]), ch)
    c["ch"] = ch
    assert (ch != CANARY).any() and (ch[:7] == CANARY).all() and (ch[-6:] == CANARY).all()
    # extraction: the REs and estimates of every segment side by side, antenna a at a * S
    rx_e, ch_e = c["rx_e"], c["ch_e"] = np.zeros((N_ANT, S, 2), np.int16), np.zeros((N_ANT, S, 2), np.int16)
    c["esegs"] = []
    for s in c["gsegs"]:
        o, nb = s["sym_off"], s["nb_re"]
        for a in range(N_ANT):
            rx_e[a, o:o + nb], ch_e[a, o:o + nb] = m.ulsch_extract_host(rx[a * rs + s["rx_off"]:a * rs + s["rx_off"] + N], ch[a * cs + s["ch_off"]:a * cs + s["ch_off"] + 12 * rb],
                                                                        s["pattern"], N, s["start_re"], nb)
        c["esegs"].append(dict(tb=0, Qm=QM, nb_re=nb, plane=S, sym_off=o, rx_off=o, ch_off=o, rec_off=s["rec_off"]))
    f = c["first"][0]
    assert f["sym_off"] == 0 and f["nb_re"] == 12 * rb
    c["lv"] = m.ulsch_level_host(ch_e.reshape(-1), N_ANT, S, f["nb_re"])[0]
    # compensation: the planes of every segment at their place in the record
    rec = np.full(2 + 2 * (QM // 2) * S + 6, CANARY, np.int16)
    for s in c["gsegs"]:
        o, nb = s["sym_off"], s["nb_re"]
        pl = m.ulsch_compensate_host(np.ascontiguousarray(rx_e[:, o:o + nb]), np.ascontiguousarray(ch_e[:, o:o + nb]), N_ANT, nb, nb, QM, c["lv"])
        for k in range(QM // 2):
            at = s["rec_off"] + 2 * (k * S + o)
            rec[at:at + 2 * nb] = pl[k].reshape(-1)
    c["rec"] = rec
    assert (rec[:2] == CANARY).all() and (rec[-6:] == CANARY).all()
    # mapping: antenna a carries layer a
    tx = np.full((N_ANT * ts, 2), CANARY, np.int16)
    for s in c["msegs"]:
        for a in range(N_ANT):
            m.pdsch_map_host(lay, dict(s, tx_off=s["tx_off"] + a * ts), a, tx)
    c["tx"] = tx
    assert (tx[0] == CANARY).all() and (tx[-4:] == CANARY).all()
    _cases[(N, rb)] = c
    return c


def run_calls(m, c, side):
    """the six calls, each HOST then DEVICE; one synchronisation at the end, so the DEVICE calls queue up behind each other"""
    import torch
    got = {}
    lv = np.array([c["lv"]], np.int32)
    with torch.cuda.stream(side):
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
        fill = lambda n, v=CANARY, dt=torch.int16: torch.full((n,), v, dtype=dt, device="cuda")
        rx_d, ch_d, rxe_d, che_d, lay_d, lv_d = dev(c["rx"]), dev(c["ch"]), dev(c["rx_e"]), dev(c["ch_e"]), dev(c["lay"]), dev(lv)
        s = side.cuda_stream
        # 1. channel estimation
        got["ch host"] = m.pusch_channel_estimation(c["rx"].reshape(-1), c["rs"], np.full(c["ch"].size, CANARY, np.int16), c["cs"], N_ANT, c["csegs"], c["delay"])
        got["ch device"] = m.pusch_channel_estimation(rx_d, c["rs"], fill(c["ch"].size), c["cs"], N_ANT, c["csegs"], dev(c["delay"]), stream=s)
        # 2. channel level from the grid's estimates
        got["lv grid host"] = m.ulsch_channel_level_grid(c["ch"].reshape(-1), N_ANT, c["cs"], c["first"])
        got["lv grid device"] = m.ulsch_channel_level_grid(ch_d, N_ANT, c["cs"], c["first"], out=fill(2, -7, torch.int32), stream=s)
        # 3. compensation from the grid
        got["rec grid host"] = m.ulsch_channel_compensation_grid(c["rx"].reshape(-1), c["ch"].reshape(-1), N_ANT, c["rs"], c["cs"], c["gsegs"], lv,
                                                                 np.full(c["rec"].size, CANARY, np.int16))
        got["rec grid device"] = m.ulsch_channel_compensation_grid(rx_d, ch_d, N_ANT, c["rs"], c["cs"], c["gsegs"], lv_d, fill(c["rec"].size), stream=s)
        # 4., 5. the same on the extracted arrays
        got["lv host"] = m.ulsch_channel_level(c["ch_e"].reshape(-1), N_ANT, c["S"], c["esegs"][:1])
        got["lv device"] = m.ulsch_channel_level(che_d, N_ANT, c["S"], c["esegs"][:1], out=fill(2, -7, torch.int32), stream=s)
        got["rec host"] = m.ulsch_channel_compensation(c["rx_e"].reshape(-1), c["ch_e"].reshape(-1), N_ANT, c["S"], c["esegs"], lv,
                                                       np.full(c["rec"].size, CANARY, np.int16))
        got["rec device"] = m.ulsch_channel_compensation(rxe_d, che_d, N_ANT, c["S"], c["esegs"], lv_d, fill(c["rec"].size), stream=s)
        # 6. resource mapping
        got["tx host"] = m.pdsch_resource_mapping(c["lay"].reshape(-1), np.full(c["tx"].size, CANARY, np.int16), c["ts"], N_ANT, c["msegs"])
        got["tx device"] = m.pdsch_resource_mapping(lay_d, fill(c["tx"].size), c["ts"], N_ANT, c["msegs"], stream=s)
    torch.cuda.synchronize()
    return {k: v if isinstance(v, np.ndarray) else v.cpu().numpy() for k, v in got.items()}


def test_calls_share_one_threads_contexts(hip):
    import torch
    m = hip.ldpc
    small, large = slot_case(m, 128, 2), slot_case(m, 2048, 106)
    # The staging buffers grow to 1.5 x the request + 4096 bytes (ThreadCtx::ensure).  The largest request of the small slot is that
    # of ulsch_channel_compensation_grid, the grid and the estimates with a few descriptors: below 32 KiB, so the first round leaves
    # at most 1.5 x 32768 + 4096 bytes.  The smallest staged input of the large slot, one symbol's extracted estimates across both
    # antennas (ulsch_channel_level), is above that: every call of the second round outgrows what the first round left, the buffers
    # are reallocated between calls of different kinds, and the third round runs in the second's buffers.
    assert small["rx"].nbytes + small["ch"].nbytes + 2048 < 32768
    assert 4 * (large["S"] + 12 * large["rb"]) > 1.5 * 32768 + 4096
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for rnd, c in enumerate((small, large, small)):
        got = run_calls(m, c, side)
        for k, v in got.items():
            want = {"ch": c["ch"], "rec": c["rec"], "tx": c["tx"]}.get(k.split()[0])
            if want is None:
                want = np.array([c["lv"]] + [-7] * (v.size - 1), np.int32)
            assert np.array_equal(v.reshape(-1), want.reshape(-1)), (rnd, k, np.flatnonzero(v.reshape(-1) != want.reshape(-1))[:8])
