"""Modulation mapping, soft demapping and the UL-SCH chain call from symbols (nrLDPC_hip_modulation / _ulsch_llr /
_ulsch_decode_symbols) against numpy and against their definition: nrLDPC_hip_ulsch_llr on each block's symbols followed by
nrLDPC_hip_ulsch_decode_scrambled."""
import ctypes as C
import os
import subprocess
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

from qam_np import demap_np, edge_symbols, mod_table_np, modulate_np
from test_gpu_tb_chain import make_tbs, valid_tbs
from test_gpu_tb_scrambled import rand_scr

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
UNIT = {2: 16384, 4: 7327, 6: 3575, 8: 1777}
SLOT_G = (12 * 13 - 6) * 273 * 6


def ideal_mags(Qm, n):
    """the magnitudes a gNB computes for a unit channel: 16QAM 2u, 64QAM 4u, 2u, 256QAM 8u, 4u, 2u (u = the inner level)"""
    u = UNIT[Qm]
    return [np.full((n, 2), (1 << (Qm // 2 - k)) * u, np.int16) for k in range(1, Qm // 2)]


def rx_symbols(rng, words, G, Qm, sigma, edges=True):
    """the points of the scrambled codeword through AWGN (sigma in units of the inner level), ideal magnitudes"""
    p = modulate_np(words, G, Qm).astype(np.float64)
    y = np.clip(np.rint(p + sigma * UNIT[Qm] * rng.standard_normal(p.shape)), -32768, 32767).astype(np.int16)
    if edges:
        y[rng.integers(0, y.shape[0], 3)] = [[-32768, 32767], [0, -32768], [32767, 0]]
    return y, ideal_mags(Qm, y.shape[0])


# ---- modulation ---------------------------------------------------------------------------------------------------------
MOD_LENGTHS = {2: [2, 6, 30, 34, 190, 1000, 2 * 12345], 4: [4, 12, 28, 36, 188, 1004, 4 * 7777],
               6: [6, 18, 42, 66, 186, 198, 6 * 13, 6 * 1001, SLOT_G], 8: [8, 24, 56, 72, 184, 200, 8 * 999]}


MOD_OFFS = (0, 1, 2)                                # int16 offsets: 16-byte, 4-byte and 2-byte aligned outputs
LLR_NB_RE = (1, 3, 4, 7, 8, 9, 100, 1001, 4096 + 3)
LLR_OFFS = (0, 2)                                   # 16-byte aligned planes and output / only 4-byte aligned ones


@pytest.mark.parametrize("Qm", [2, 4, 6, 8])
def test_modulation_host_and_device_against_numpy(hip, Qm):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(100 + Qm)
    for length in MOD_LENGTHS[Qm]:
        nw = (length + 31) // 32
        words = rng.integers(0, 1 << 32, nw + 1, dtype=np.uint64).astype(np.uint32)
        want = modulate_np(words, length, Qm)
        got = m.modulation(words[:nw], length, Qm)
        assert np.array_equal(got, want), (Qm, length)
        for off in MOD_OFFS:
            out = torch.full((2 * (length // Qm) + off + 8,), 0x5a5a, dtype=torch.int16, device="cuda")
            m.modulation(torch.from_numpy(words[:nw].view(np.int32)).cuda(), length, Qm, out=out[off:])
            torch.cuda.synchronize()
            o = out.cpu().numpy()
            assert np.array_equal(o[off:off + 2 * (length // Qm)].reshape(-1, 2), want), (Qm, length, off)
            assert (o[:off] == 0x5a5a).all() and (o[off + 2 * (length // Qm):] == 0x5a5a).all(), (Qm, length, off)


# ---- soft demapping -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Qm", [2, 4, 6, 8])
def test_ulsch_llr_host_and_device_against_numpy(hip, Qm):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(200 + Qm)
    for nb_re in LLR_NB_RE:
        y, mags = edge_symbols(rng, nb_re, Qm)
        want = demap_np(y, mags, Qm)
        assert np.array_equal(m.ulsch_llr(y, mags, Qm), want), (Qm, nb_re)
        for off in LLR_OFFS:
            dev = []
            for a in [y] + mags:
                t = torch.zeros(2 * nb_re + off, dtype=torch.int16, device="cuda")
                t[off:] = torch.from_numpy(a.reshape(-1)).cuda()
                dev.append(t[off:])
            out = torch.full((nb_re * Qm + off + 16,), 0x5a5a, dtype=torch.int16, device="cuda")
            m.ulsch_llr(dev[0], dev[1:], Qm, out=out[off:])
            torch.cuda.synchronize()
            o = out.cpu().numpy()
            assert np.array_equal(o[off:off + nb_re * Qm], want), (Qm, nb_re, off)
            assert (o[:off] == 0x5a5a).all() and (o[off + nb_re * Qm:] == 0x5a5a).all(), (Qm, nb_re, off)


# ---- decode_symbols = ulsch_llr + decode_scrambled ----------------------------------------------------------------------
def sym_tbs():
    tbs = [t for t in make_tbs() if t["A"] < 60000]                  # mixes Qm, BG, LBRM, Nl = 2
    return tbs


def block_records(rng, m, tbs, scr, pays, sigma):
    tx = m.dlsch_encode_scrambled_host(tbs, pays, scr)
    syms = [rx_symbols(rng, w, t["G"], t["Qm"], sigma) for w, t in zip(tx, tbs)]
    recs = m.pack_symbol_records([[y] + mg for y, mg in syms])
    llrs = [m.ulsch_llr(y, mg, t["Qm"]) for (y, mg), t in zip(syms, tbs)]
    return recs, llrs


@pytest.mark.parametrize("mode", ["device", "host", "pinned", "harq_device", "harq_library"])
def test_decode_symbols_equals_llr_then_decode_scrambled(hip, mode):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(zlib.crc32(mode.encode()) + 1)
    tbs = sym_tbs()
    n = len(tbs)
    scr = rand_scr(rng, n)
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
    po, co, ho, segs = m.tb_layout(tbs)
    llrlen_a, llrlen_b = [0] * n, [0] * n
    harq_a = np.zeros(int(ho[-1]) + 16, np.int16)
    harq_b = harq_a.copy()
    ids_a = [3000 + i for i in range(n)]
    ids_b = [4000 + i for i in range(n)]
    for rnd, (rv, sigma) in enumerate(((0, 0.45), (2, 0.25))):
        cur = [dict(t, rv=rv) for t in tbs]
        recs, llrs = block_records(rng, m, cur, scr, pays, sigma)
        recs_copy = [r.copy() for r in recs]
        rx_a = [dict(t, round=rnd, llrLen=llrlen_a[i]) for i, t in enumerate(cur)]
        rx_b = [dict(t, round=rnd, llrLen=llrlen_b[i]) for i, t in enumerate(cur)]
        if mode == "device":
            def run(rx, L, harq, fn, **kw):
                src = torch.zeros(int(co[-1]) + 16, dtype=torch.int16)
                for i, x in enumerate(L):
                    src[co[i]:co[i] + x.size] = torch.from_numpy(x)
                src = src.cuda()
                before = src.clone()
                h = torch.from_numpy(harq).cuda()
                pay = torch.zeros(int(po[-1]) + 16, dtype=torch.uint8, device="cuda")
                ack = torch.zeros(n, dtype=torch.uint8, device="cuda")
                itm = torch.zeros(n, dtype=torch.int32, device="cuda")
                fn(rx, src, h, pay, ack, itm, **kw)
                torch.cuda.synchronize()
                assert torch.equal(src, before)
                harq[:] = h.cpu().numpy()
                ph = pay.cpu().numpy()
                return [ph[po[i]:po[i] + t["A"] // 8] for i, t in enumerate(rx)], ack.cpu().numpy().astype(bool), itm.cpu().numpy()
            out_b = run(rx_b, llrs, harq_b, m.ulsch_decode_scrambled_device, scrambling=scr)
            out_a = run(rx_a, recs, harq_a, m.ulsch_decode_symbols_device, scrambling=scr)
        else:
            kw = dict(pinned=(mode == "pinned"))
            if mode == "harq_library":
                out_b = m.ulsch_decode_scrambled_host(rx_b, llrs, None, scr, harq_ids=ids_b)
                out_a = m.ulsch_decode_symbols_host(rx_a, recs, None, scr, harq_ids=ids_a)
            elif mode == "harq_device":
                hb, ha = torch.from_numpy(harq_b).cuda(), torch.from_numpy(harq_a).cuda()
                out_b = m.ulsch_decode_scrambled_host(rx_b, llrs, hb, scr)
                out_a = m.ulsch_decode_symbols_host(rx_a, recs, ha, scr)
                harq_b[:], harq_a[:] = hb.cpu().numpy(), ha.cpu().numpy()
            else:
                out_b = m.ulsch_decode_scrambled_host(rx_b, llrs, harq_b, scr, **kw)
                out_a = m.ulsch_decode_symbols_host(rx_a, recs, harq_a, scr, **kw)
        for x, y in zip(recs, recs_copy):
            assert np.array_equal(x, y)                                   # the records are only read
        for i in range(n):
            assert np.array_equal(out_a[0][i], out_b[0][i]), (mode, rnd, i)
        assert np.array_equal(out_a[1], out_b[1]) and np.array_equal(out_a[2], out_b[2]), (mode, rnd)
        assert [t["llrLen"] for t in rx_a] == [t["llrLen"] for t in rx_b]
        if mode == "harq_library":
            for i in range(n):
                ha = m.harq_read(ids_a[i], segs[i] * m.HARQ_STRIDE)
                hb = m.harq_read(ids_b[i], segs[i] * m.HARQ_STRIDE)
                assert np.array_equal(ha, hb), (rnd, i)
        else:
            assert np.array_equal(harq_a, harq_b), (mode, rnd)
        llrlen_a = [t["llrLen"] for t in rx_a]
        llrlen_b = [t["llrLen"] for t in rx_b]
        assert out_a[1].sum() > 0, (mode, rnd)
    if mode == "harq_library":
        m.harq_release()


@pytest.mark.parametrize("env", [{"NRLDPC_HIP_TB_FUSED": "0"}, {"NRLDPC_HIP_TB_MULTI": "2"}])
def test_decode_symbols_other_rx_paths(hip, env):
    """the four-launch path, and small segments sharing workgroups (both through tb_rx_dematch_sym_kernel)"""
    if any(os.environ.get(k) == v for k, v in env.items()):
        pytest.skip("already this configuration")
    r = subprocess.run([sys.executable, "-m", "pytest", str(HERE / "test_gpu_qam.py"), "-m", "gpu", "-q", "-x", "-k",
                        "test_decode_symbols_equals_llr_then_decode_scrambled and (device or host) or test_small_symbol_blocks"],
                       env=dict(os.environ, **env), cwd=str(HERE.parent), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_small_symbol_blocks_share_workgroups(hip):
    m = hip.ldpc
    rng = np.random.default_rng(98)
    tbs = []
    for A in (24, 104, 336, 808, 1544, 3104, 3824):
        for _ in range(4):
            Qm = int(rng.choice([2, 4, 6, 8]))
            tbs.append(dict(A=A, G=max(int(A / 0.4) // Qm, 4) * Qm, BG=2, Qm=Qm, Nl=1, rv=0, tbslbrm=0))
    scr = rand_scr(rng, len(tbs))
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
    recs, llrs = block_records(rng, m, tbs, scr, pays, 0.25)
    harq_a = np.zeros((len(tbs), m.HARQ_STRIDE), np.int16)
    harq_b = harq_a.copy()
    a = m.ulsch_decode_symbols_host([dict(t, round=0, llrLen=0) for t in tbs], recs, harq_a, scr)
    b = m.ulsch_decode_scrambled_host([dict(t, round=0, llrLen=0) for t in tbs], llrs, harq_b, scr)
    for i in range(len(tbs)):
        assert np.array_equal(a[0][i], b[0][i]), i
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(harq_a, harq_b)
    assert a[1].sum() > len(tbs) // 2


def test_decode_symbols_sharded_over_logical_devices(hip, tmp_path):
    outs = []
    for devs in (None, "0,0,0"):
        env = dict(os.environ)
        env.pop("NRLDPC_HIP_DEVICES", None)
        if devs:
            env["NRLDPC_HIP_DEVICES"] = devs
        f = tmp_path / f"out_{devs or 'single'}.npz"
        r = subprocess.run([sys.executable, str(HERE / "multidev_symbols_script.py"), str(f)], capture_output=True, text=True, env=env,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(np.load(f))
    a, b = outs
    assert sorted(a.files) == sorted(b.files) and len(a.files) >= 6
    for k in a.files:
        assert np.array_equal(a[k], b[k]), k
    assert a["ok"].all()


# ---- end to end on device buffers ---------------------------------------------------------------------------------------
def e2e(m, rng, tbs, sigma):
    import torch
    scr = rand_scr(rng, len(tbs))
    po, co, ho, _ = m.tb_layout(tbs)
    cw, total = m.tb_layout_packed(tbs)
    pay_h = rng.integers(0, 256, int(po[-1]) + 16, dtype=np.uint8)
    payload = torch.from_numpy(pay_h).cuda()
    words = torch.zeros(total // 4 + 4, dtype=torch.int32, device="cuda")
    m.dlsch_encode_scrambled_device(tbs, payload, words, scr)
    pts = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")
    for i, t in enumerate(tbs):                                        # the points in the first plane of each record
        m.modulation(words[cw[i] // 4:], t["G"], t["Qm"], out=pts[co[i]:])
    torch.cuda.synchronize()
    ph = pts.cpu().numpy()
    rec_h = np.zeros_like(ph)
    for i, t in enumerate(tbs):
        S = t["G"] // t["Qm"]
        p = ph[co[i]:co[i] + 2 * S].astype(np.float64)
        y = np.clip(np.rint(p + sigma * UNIT[t["Qm"]] * rng.standard_normal(p.shape)), -32768, 32767).astype(np.int16)
        rec_h[co[i]:co[i] + t["G"]] = m.pack_symbol_records([[y] + ideal_mags(t["Qm"], S)])[0]
    rec = torch.from_numpy(rec_h).cuda()
    harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
    pay_out = torch.zeros_like(payload)
    ack = torch.zeros(len(tbs), dtype=torch.uint8, device="cuda")
    itm = torch.zeros(len(tbs), dtype=torch.int32, device="cuda")
    m.ulsch_decode_symbols_device([dict(t, round=0, llrLen=0) for t in tbs], rec, harq, pay_out, ack, itm, scr)
    torch.cuda.synchronize()
    out = pay_out.cpu().numpy()
    assert ack.cpu().numpy().all()
    for i, t in enumerate(tbs):
        assert np.array_equal(out[po[i]:po[i] + t["A"] // 8], pay_h[po[i]:po[i] + t["A"] // 8]), i


@pytest.mark.parametrize("Qm", [2, 4, 6, 8])
def test_end_to_end_modulation_awgn_decode_symbols(hip, Qm):
    rng = np.random.default_rng(500 + Qm)
    tbs = [dict(A=valid_tbs(20000, 1), G=Qm * 12000, BG=1, Qm=Qm, Nl=1, rv=0, tbslbrm=0),
           dict(A=valid_tbs(3000, 2), G=Qm * 3000, BG=2, Qm=Qm, Nl=2, rv=0, tbslbrm=0)]
    e2e(hip.ldpc, rng, tbs, 0.15)


def test_end_to_end_64_block_slot(hip):
    t0 = dict(A=valid_tbs(213176, 1), G=SLOT_G, BG=1, Qm=6, Nl=1, rv=0, tbslbrm=0)
    e2e(hip.ldpc, np.random.default_rng(64), [dict(t0) for _ in range(64)], 0.15)


# ---- plans and graphs ---------------------------------------------------------------------------------------------------
def test_symbol_plans_and_graphs(hip):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(6160)
    tbs = [dict(t, round=0, llrLen=0) for t in sym_tbs()[:5]]
    n = len(tbs)
    scr = rand_scr(rng, n)
    po, co, ho, _ = m.tb_layout(tbs)
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
    recs, llrs = block_records(rng, m, tbs, scr, pays, 0.15)
    rec = torch.zeros(int(co[-1]) + 16, dtype=torch.int16)
    llr = torch.zeros(int(co[-1]) + 16, dtype=torch.int16)
    for i in range(n):
        rec[co[i]:co[i] + recs[i].size] = torch.from_numpy(recs[i])
        llr[co[i]:co[i] + llrs[i].size] = torch.from_numpy(llrs[i])
    rec, llr = rec.cuda(), llr.cuda()
    harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
    pay_s, pay_l = (torch.zeros(int(po[-1]) + 16, dtype=torch.uint8, device="cuda") for _ in range(2))
    ack_s, ack_l = (torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(2))
    itm = torch.zeros(n, dtype=torch.int32, device="cuda")
    # the same descriptors, alternating: a symbol call on the LLR array must not reuse the LLR call's plan, nor the reverse
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dec_s = m.PreparedTbBatch(tbs, pay_s, rec, harq, ack_s, itm, scrambling=scr, symbols=True)
        dec_l = m.PreparedTbBatch(tbs, pay_l, llr, harq, ack_l, itm, scrambling=scr)
        for _ in range(3):
            dec_s.decode()
            dec_l.decode()
    torch.cuda.synchronize()
    for p, a in ((pay_s, ack_s), (pay_l, ack_l)):
        assert a.cpu().numpy().all()
        ph = p.cpu().numpy()
        for i, t in enumerate(tbs):
            assert np.array_equal(ph[po[i]:po[i] + t["A"] // 8], pays[i]), i
    # a symbol call given LLRs is a different computation: it must not decode (a plan shared with the LLR call would)
    bad = m.PreparedTbBatch(tbs, pay_s, llr, harq, ack_s, itm, scrambling=scr, symbols=True)
    with torch.cuda.stream(side):
        ack_s.fill_(7)
        bad.decode()
    torch.cuda.synchronize()
    assert not ack_s.cpu().numpy().all()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        dec_s.decode()
    for rep in range(2):
        pays2 = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
        recs2, _ = block_records(rng, m, tbs, scr, pays2, 0.15)
        for i in range(n):
            rec[co[i]:co[i] + recs2[i].size] = torch.from_numpy(recs2[i]).cuda()
        pay_s.zero_()
        ack_s.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert ack_s.cpu().numpy().all(), rep
        ph = pay_s.cpu().numpy()
        for i, t in enumerate(tbs):
            assert np.array_equal(ph[po[i]:po[i] + t["A"] // 8], pays2[i]), (rep, i)


# ---- invalid input ------------------------------------------------------------------------------------------------------
def test_qam_invalid_input(hip):
    import torch
    m = hip.ldpc
    L, T = m._qam_lib(), m._tb_lib()
    words = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.full((1024,), 0x5a5a, dtype=torch.int16, device="cuda")
    for length, Qm, why in ((96, 3, "Qm"), (100, 6, "multiple of Qm"), ((1 << 21) + 8, 8, "2^21")):
        assert L.nrLDPC_hip_modulation(words.data_ptr(), length, Qm, out.data_ptr(), m.MEM_DEVICE, None) < 0
        assert why in m.last_error()
    assert L.nrLDPC_hip_modulation(None, 96, 4, out.data_ptr(), m.MEM_DEVICE, None) < 0
    assert L.nrLDPC_hip_modulation(words.data_ptr(), 96, 4, None, m.MEM_DEVICE, None) < 0
    assert L.nrLDPC_hip_modulation(words.data_ptr(), 96, 4, out.data_ptr(), 7, None) < 0
    y = torch.zeros(64, dtype=torch.int32, device="cuda")
    assert L.nrLDPC_hip_ulsch_llr(y.data_ptr(), None, None, None, 64, 4, out.data_ptr(), m.MEM_DEVICE, None) < 0   # NULL mag_a
    assert L.nrLDPC_hip_ulsch_llr(y.data_ptr(), y.data_ptr(), None, None, 64, 5, out.data_ptr(), m.MEM_DEVICE, None) < 0
    assert L.nrLDPC_hip_ulsch_llr(y.data_ptr(), y.data_ptr(), None, None, (1 << 19) + 1, 4, out.data_ptr(), m.MEM_DEVICE, None) < 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5a5a).all()
    # decode_symbols: NULL scr, G % Qm, odd coded_off, bad Qm -- nothing written
    pay = np.zeros(128, np.uint8)
    rec = np.ones(4096, np.int16)
    for t, off, scr, why in ((dict(A=800, G=2400, BG=2, Qm=2, Nl=1), 0, None, "scr is NULL"),
                             (dict(A=800, G=2402, BG=2, Qm=4, Nl=1), 0, [(1, 0, 1)], "multiple of Qm"),
                             (dict(A=800, G=2400, BG=2, Qm=2, Nl=1), 1, [(1, 0, 1)], "even"),
                             (dict(A=800, G=2400, BG=2, Qm=3, Nl=1), 0, [(1, 0, 1)], "Qm"),
                             (dict(A=800, G=2400, BG=2, Qm=2, Nl=1), 0, [(1, 2, 1)], "q")):
        harq = np.full(m.HARQ_STRIDE, 7, np.int16)
        ack = np.full(1, 9, np.uint8)
        itm = np.full(1, 9, np.int32)
        arr = m._tb_array([dict(t, round=0)], [0], [off], [0])
        b = m.nrLDPC_hip_tb_batch_t(n_tb=1, tb=arr, payload=pay.ctypes.data, coded=rec.ctypes.data, harq=harq.ctypes.data,
                                    harq_stride=m.HARQ_STRIDE, ack=ack.ctypes.data, iter_max=itm.ctypes.data, mem=m.MEM_HOST, stream=None)
        assert T.nrLDPC_hip_ulsch_decode_symbols(C.byref(b), None if scr is None else m._scr_array(scr, 1)) < 0, why
        assert why in m.last_error(), (why, m.last_error())
        assert (harq == 7).all() and ack[0] == 9 and itm[0] == 9 and (pay == 0).all()
    # a record that is not 4-byte aligned
    arr = m._tb_array([dict(A=800, G=2400, BG=2, Qm=2, Nl=1, round=0)], [0], [0], [0])
    b = m.nrLDPC_hip_tb_batch_t(n_tb=1, tb=arr, payload=pay.ctypes.data, coded=rec.ctypes.data + 2, harq=harq.ctypes.data,
                                harq_stride=m.HARQ_STRIDE, ack=ack.ctypes.data, iter_max=itm.ctypes.data, mem=m.MEM_HOST, stream=None)
    assert T.nrLDPC_hip_ulsch_decode_symbols(C.byref(b), m._scr_array([(1, 0, 1)], 1)) < 0 and "4-byte" in m.last_error()
    assert (harq == 7).all() and ack[0] == 9
