"""The DL-SCH chain call to layer-mapped symbols (nrLDPC_hip_dlsch_encode_symbols) and the standalone layer mapping
(nrLDPC_hip_layer_mapping) against their definition: the scrambled encode call, then modulation, then nr_layer_mapping
(numpy: tests/layer_np.py), every TB its own codeword."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as O
from layer_np import layer_demap_np, layer_map_np, symbols_np
from qam_np import modulate_np
from test_gpu_qam import ideal_mags
from test_gpu_tb_chain import make_tbs, valid_tbs
from test_gpu_tb_scrambled import encode_cases, rand_scr, scrambled_words

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
SENT = 0x5a5a5a5a


def sym_cases():
    """make_tbs() (Nl 1, 2, 4), the big / tiny / odd blocks of the scrambled tests, and three-layer blocks (a layer group can
    straddle two selection chunks: 2048 symbols per chunk)"""
    nl3 = [dict(A=valid_tbs(40000, 1), G=6 * 3 * 3001, BG=1, Qm=6, Nl=3, rv=0, tbslbrm=0),
           dict(A=valid_tbs(8000, 1), G=4 * 3 * 2100, BG=1, Qm=4, Nl=3, rv=1, tbslbrm=0),
           dict(A=valid_tbs(3000, 2), G=2 * 3 * 4001, BG=2, Qm=2, Nl=3, rv=0, tbslbrm=0),
           dict(A=valid_tbs(50000, 1), G=8 * 3 * 2500, BG=1, Qm=8, Nl=3, rv=2, tbslbrm=0)]
    return encode_cases() + nl3


def gapped_offsets(tbs, gap=20):
    """byte offsets with `gap` bytes between the blocks' records (4-byte aligned, mostly not 16-byte aligned) and the total"""
    co = np.cumsum([0] + [4 * (t["G"] // t["Qm"]) + gap for t in tbs])
    return [int(x) for x in co[:-1]], int(co[-1])


def want_symbols(m, tbs, pays, scr):
    bits = m.dlsch_encode_host(tbs, pays)
    return [symbols_np(f, s, t["Qm"], t["Nl"]) for f, s, t in zip(bits, scr, tbs)]


def check_record(out32, offs, tbs, want, what):
    """every block's planes equal, every word outside them the sentinel"""
    mask = np.ones(out32.size, bool)
    for i, t in enumerate(tbs):
        S = t["G"] // t["Qm"]
        w0 = offs[i] // 4
        got = out32[w0:w0 + S].view(np.int16).reshape(t["Nl"], S // t["Nl"], 2)
        assert np.array_equal(got, want[i]), (what, i)
        mask[w0:w0 + S] = False
    assert (out32[mask] == SENT).all(), what


def encode_host_raw(m, tbs, pays, scr, offs, total, pinned):
    """nrLDPC_hip_dlsch_encode_symbols on host buffers (pageable numpy, or page-locked PinnedArray), sentinels around the blocks"""
    L = m._tb_lib()
    po = np.cumsum([0] + [(t["A"] // 8 + 15) // 16 * 16 for t in tbs])
    keep = []
    if pinned:
        pay_k, out_k = m.PinnedArray(int(po[-1]) + 16, np.uint8), m.PinnedArray(total // 4 + 8, np.uint32)
        pay, out = pay_k.a, out_k.a
        keep = [pay_k, out_k]
    else:
        pay, out = np.zeros(int(po[-1]) + 16, np.uint8), np.zeros(total // 4 + 8, np.uint32)
    pay[:] = 0
    out[:] = SENT
    for i, p in enumerate(pays):
        pay[po[i]:po[i] + tbs[i]["A"] // 8] = p
    arr = m._tb_array(tbs, po, offs, None)
    b = m.nrLDPC_hip_tb_batch_t(n_tb=len(tbs), tb=arr, payload=pay.ctypes.data, coded=out.ctypes.data, harq=None, harq_stride=0,
                                ack=None, iter_max=None, mem=m.MEM_HOST, stream=None)
    assert L.nrLDPC_hip_dlsch_encode_symbols(C.byref(b), m._scr_array(scr, len(tbs))) == 0, m.last_error()
    res = out.copy()
    del keep
    return res


def test_encode_symbols_equals_scrambled_modulation_layer_mapping(hip):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(9311)
    tbs = sym_cases()
    scr = rand_scr(rng, len(tbs))
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
    want = want_symbols(m, tbs, pays, scr)
    # host buffers, the wrapper's layout
    got = m.dlsch_encode_symbols_host(tbs, pays, scr)
    for i in range(len(tbs)):
        assert np.array_equal(got[i], want[i]), i
    # host buffers, pageable and page-locked, sentinels between the blocks
    offs, total = gapped_offsets(tbs)
    for pinned in (False, True):
        check_record(encode_host_raw(m, tbs, pays, scr, offs, total, pinned), offs, tbs, want, f"host pinned={pinned}")
    # device buffers, sentinels between the blocks
    po, _, _, _ = m.tb_layout(tbs)
    pay_h = np.zeros(int(po[-1]) + 16, np.uint8)
    for i, t in enumerate(tbs):
        pay_h[po[i]:po[i] + t["A"] // 8] = pays[i]
    coded = torch.full((total // 4 + 8,), SENT, dtype=torch.int32, device="cuda")
    m.dlsch_encode_symbols_device(tbs, torch.from_numpy(pay_h).cuda(), coded, scr, coded_off=offs)
    torch.cuda.synchronize()
    check_record(coded.cpu().numpy().view(np.uint32), offs, tbs, want, "device")
    # ... and the library's own three calls give the same bytes (encode_scrambled -> modulation -> layer_mapping)
    cw, wtot = m.tb_layout_packed(tbs)
    words = torch.zeros(wtot // 4 + 4, dtype=torch.int32, device="cuda")
    m.dlsch_encode_scrambled_device(tbs, torch.from_numpy(pay_h).cuda(), words, scr)
    for i, t in enumerate(tbs[:8]):
        S = t["G"] // t["Qm"]
        pts = torch.zeros(2 * S, dtype=torch.int16, device="cuda")
        m.modulation(words[cw[i] // 4:], t["G"], t["Qm"], out=pts)
        planes = torch.zeros(2 * S, dtype=torch.int16, device="cuda")
        m.layer_mapping(pts, t["Nl"], out=planes)
        torch.cuda.synchronize()
        assert np.array_equal(planes.cpu().numpy().reshape(t["Nl"], S // t["Nl"], 2), want[i]), i


@pytest.mark.parametrize("env", [{"NRLDPC_HIP_ENC_KERNEL": "bytes"}, {"NRLDPC_HIP_TB_TRUNC": "0"}])
def test_encode_symbols_other_tx_paths(hip, env):
    if any(os.environ.get(k) == v for k, v in env.items()):
        pytest.skip("already this configuration")
    r = subprocess.run([sys.executable, "-m", "pytest", str(HERE / "test_gpu_dl_symbols.py"), "-m", "gpu", "-q", "-x", "-k",
                        "test_encode_symbols_equals_scrambled_modulation_layer_mapping or test_symbol_plans_and_graphs"],
                       env=dict(os.environ, **env), cwd=str(HERE.parent), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


LAYER_PER = (1, 3, 4, 5, 64, 1001, 4096 + 7)        # points per layer
LAYER_OFFS = ((0, 0), (2, 2), (1, 2), (0, 1))       # int16 offsets of in and out: 16-byte, 4-byte, 2-byte aligned arrays


def layer_strides(per):
    return (per, per + 3, per + 4)


@pytest.mark.parametrize("Nl", [1, 2, 3, 4])
def test_layer_mapping_host_and_device_against_numpy(hip, Nl):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(500 + Nl)
    for per in LAYER_PER:
        n = per * Nl
        pts = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
        want = layer_map_np(pts, Nl)
        for stride in layer_strides(per):
            got = m.layer_mapping(pts, Nl, layer_stride=stride)
            assert np.array_equal(got[:, :per], want), (Nl, per, stride)
            assert (got[:, per:] == 0).all()
            # the library's own output array with sentinels between the planes (host: nothing else of `out` is written)
            out = np.full((Nl * stride + 4) * 2, 0x5a5a, np.int16)
            L = m._qam_lib()
            assert L.nrLDPC_hip_layer_mapping(pts.ctypes.data, n, Nl, out.ctypes.data, stride, m.MEM_HOST, None) == 0
            o = out[:Nl * stride * 2].reshape(Nl, stride, 2)
            assert np.array_equal(o[:, :per], want) and (o[:, per:] == 0x5a5a).all() and (out[Nl * stride * 2:] == 0x5a5a).all()
            for off_in, off_out in LAYER_OFFS:
                src = torch.zeros(2 * n + 8, dtype=torch.int16, device="cuda")
                x = src[off_in:off_in + 2 * n]
                x.copy_(torch.from_numpy(pts.reshape(-1)).cuda())
                dst = torch.full((2 * Nl * stride + 8,), 0x5a5a, dtype=torch.int16, device="cuda")
                m.layer_mapping(x, Nl, out=dst[off_out:], layer_stride=stride)
                torch.cuda.synchronize()
                d = dst.cpu().numpy()
                assert (d[:off_out] == 0x5a5a).all()
                o = d[off_out:off_out + 2 * Nl * stride].reshape(Nl, stride, 2)
                assert np.array_equal(o[:, :per], want), (Nl, per, stride, off_in, off_out)
                assert (o[:, per:] == 0x5a5a).all() and (d[off_out + 2 * Nl * stride:] == 0x5a5a).all()


def test_encode_symbols_sharded_over_logical_devices(hip, tmp_path):
    outs = []
    for devs in (None, "0,0,0"):
        env = dict(os.environ)
        env.pop("NRLDPC_HIP_DEVICES", None)
        if devs:
            env["NRLDPC_HIP_DEVICES"] = devs
        f = tmp_path / f"out_{devs or 'single'}.npz"
        r = subprocess.run([sys.executable, str(HERE / "multidev_dl_symbols_script.py"), str(f)], capture_output=True, text=True, env=env,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(np.load(f))
    a, b = outs
    assert sorted(a.files) == sorted(b.files) and len(a.files) >= 3
    for k in a.files:
        assert np.array_equal(a[k], b[k]), k
    assert a["ok"].all()


def test_symbol_plans_and_graphs(hip):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(6150)
    tbs = [dict(t, round=0, llrLen=0) for t in make_tbs()[:7]] + [dict(sym_cases()[-4], round=0, llrLen=0)]
    scr = rand_scr(rng, len(tbs))
    po, _, _, _ = m.tb_layout(tbs)
    cw, wtot = m.tb_layout_packed(tbs)
    cs, stot = m.tb_layout_symbols(tbs)
    pay_h = rng.integers(0, 256, int(po[-1]) + 16, dtype=np.uint8)
    payload = torch.from_numpy(pay_h).cuda()
    words = torch.zeros(wtot // 4 + 4, dtype=torch.int32, device="cuda")
    syms = torch.zeros(stot // 4 + 4, dtype=torch.int32, device="cuda")
    bits = [O.dlsch_encode(t, pay_h[po[i]:po[i] + t["A"] // 8]) for i, t in enumerate(tbs)]
    want_w = [scrambled_words(f, *s) for f, s in zip(bits, scr)]
    want = [symbols_np(f, s, t["Qm"], t["Nl"]) for f, s, t in zip(bits, scr, tbs)]
    # symbol and scrambled calls alternating on the same descriptors: neither takes the other's plan
    for k in range(3):
        words.zero_()
        syms.zero_()
        m.dlsch_encode_symbols_device(tbs, payload, syms, scr)
        m.dlsch_encode_scrambled_device(tbs, payload, words, scr)
        torch.cuda.synchronize()
        wv, sv = words.cpu().numpy().view(np.uint32), syms.cpu().numpy().view(np.uint32)
        for i, t in enumerate(tbs):
            S, nw = t["G"] // t["Qm"], (t["G"] + 31) // 32
            assert np.array_equal(sv[cs[i] // 4:cs[i] // 4 + S].view(np.int16).reshape(t["Nl"], S // t["Nl"], 2), want[i]), (k, i)
            assert np.array_equal(wv[cw[i] // 4:cw[i] // 4 + nw], want_w[i]), (k, i)
            assert np.array_equal(layer_map_np(modulate_np(want_w[i], t["G"], t["Qm"]), t["Nl"]), want[i]), (k, i)
    # a HIP graph of PreparedTbBatch(symbols=True).encode() replays to the right bytes for new payloads
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        enc = m.PreparedTbBatch(tbs, payload, syms, scrambling=scr, symbols=True)
        for _ in range(3):
            enc.encode()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        enc.encode()
    for rep in range(2):
        ph = rng.integers(0, 256, int(po[-1]) + 16, dtype=np.uint8)
        payload.copy_(torch.from_numpy(ph))
        syms.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        sv = syms.cpu().numpy().view(np.uint32)
        for i, t in enumerate(tbs):
            S = t["G"] // t["Qm"]
            w = symbols_np(O.dlsch_encode(t, ph[po[i]:po[i] + t["A"] // 8]), scr[i], t["Qm"], t["Nl"])
            assert np.array_equal(sv[cs[i] // 4:cs[i] // 4 + S].view(np.int16).reshape(t["Nl"], S // t["Nl"], 2), w), (rep, i)


def records_from_planes(planes, Qm, gain=0.25):
    """the UL symbol record of a noiseless reception through a channel of amplitude `gain`: y = the transmitted points in
    codeword order times gain, the ideal magnitudes times gain (at gain 1 the outer 64QAM / 256QAM points give LLRs whose
    int16 soft-buffer sums wrap where the circular buffer repeats, as the reference's do)"""
    y = np.rint(layer_demap_np(planes).astype(np.float64) * gain).astype(np.int16)
    return [y] + [np.rint(mg.astype(np.float64) * gain).astype(np.int16) for mg in ideal_mags(Qm, y.shape[0])]


def test_round_trip_through_decode_symbols(hip):
    """encode to symbols, layer-demap, ideal channel magnitudes, ulsch_decode_symbols: every block ACKs with its payload"""
    m = hip.ldpc
    rng = np.random.default_rng(77)
    tbs = [dict(t, rv=0) for t in make_tbs() if t["A"] < 60000] + [dict(t, rv=0) for t in sym_cases()[-4:]]
    scr = rand_scr(rng, len(tbs))
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
    planes = m.dlsch_encode_symbols_host(tbs, pays, scr)
    recs = m.pack_symbol_records([records_from_planes(p, t["Qm"]) for p, t in zip(planes, tbs)])
    segs = [m.nr_segmentation(t["A"] + (24 if t["A"] > 3824 else 16), t["BG"])["C"] for t in tbs]
    harq = np.zeros((sum(segs), m.HARQ_STRIDE), np.int16)
    rx = [dict(t, round=0, llrLen=0) for t in tbs]
    out, ack, _ = m.ulsch_decode_symbols_host(rx, recs, harq, scr)
    assert ack.all(), ack
    for i in range(len(tbs)):
        assert np.array_equal(out[i], pays[i]), i


def test_slot_round_trip_64_blocks_on_device(hip):
    """The 64-TB slot (BASELINE configs[3]) with 1 and 2 layers, device buffers: encode to symbols, layer-demap, decode from
    symbols; every block ACKed with its payload.  One layer: the output is the modulation output of the scrambled words."""
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(640)
    for Nl in (1, 2):
        t0 = dict(A=valid_tbs(213176, 1), G=(12 * 13 - 6) * 273 * 6, BG=1, Qm=6, Nl=Nl, rv=0, tbslbrm=0)
        tbs = [dict(t0) for _ in range(64)]
        scr = rand_scr(rng, 64)
        po, co, ho, _ = m.tb_layout(tbs)
        cs, stot = m.tb_layout_symbols(tbs)
        S = t0["G"] // 6
        pay_h = rng.integers(0, 256, int(po[-1]) + 16, dtype=np.uint8)
        payload = torch.from_numpy(pay_h).cuda()
        syms = torch.full((stot // 4 + 4,), SENT, dtype=torch.int32, device="cuda")
        m.dlsch_encode_symbols_device(tbs, payload, syms, scr)
        if Nl == 1:
            cw, wtot = m.tb_layout_packed(tbs)
            words = torch.zeros(wtot // 4 + 4, dtype=torch.int32, device="cuda")
            m.dlsch_encode_scrambled_device(tbs, payload, words, scr)
            pts = torch.full_like(syms, SENT)
            for i in range(64):
                m.modulation(words[cw[i] // 4:], t0["G"], 6, out=pts[cs[i] // 4:].view(torch.int16))
            torch.cuda.synchronize()
            assert torch.equal(pts, syms)
        sv = syms.cpu().numpy().view(np.uint32)
        rec_h = np.zeros(int(co[-1]) + 16, np.int16)
        for i in range(64):
            planes = sv[cs[i] // 4:cs[i] // 4 + S].view(np.int16).reshape(Nl, S // Nl, 2)
            rec_h[co[i]:co[i] + t0["G"]] = m.pack_symbol_records([records_from_planes(planes, 6)])[0]
        rec = torch.from_numpy(rec_h).cuda()
        harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
        pay_out = torch.zeros_like(payload)
        ack = torch.zeros(64, dtype=torch.uint8, device="cuda")
        itm = torch.zeros(64, dtype=torch.int32, device="cuda")
        rx = [dict(t, round=0, llrLen=0) for t in tbs]
        m.ulsch_decode_symbols_device(rx, rec, harq, pay_out, ack, itm, scr)
        torch.cuda.synchronize()
        assert ack.cpu().numpy().all(), Nl
        out = pay_out.cpu().numpy()
        for i in range(64):
            assert np.array_equal(out[po[i]:po[i] + t0["A"] // 8], pay_h[po[i]:po[i] + t0["A"] // 8]), (Nl, i)


def test_symbols_invalid_input(hip):
    import torch
    m = hip.ldpc
    L = m._tb_lib()
    Lq = m._qam_lib()
    pay = np.zeros(256, np.uint8)

    def call(tbs, offs, scr, base=0, mem=None, refused=True):
        out = np.full(4096, SENT, np.uint32)
        arr = m._tb_array(tbs, [0] * len(tbs), offs, None)
        b = m.nrLDPC_hip_tb_batch_t(n_tb=len(tbs), tb=arr, payload=pay.ctypes.data, coded=out.ctypes.data + base, harq=None,
                                    harq_stride=0, ack=None, iter_max=None, mem=m.MEM_HOST if mem is None else mem, stream=None)
        rc = L.nrLDPC_hip_dlsch_encode_symbols(C.byref(b), scr)
        if refused:
            assert (out == SENT).all()                                    # nothing written
        return rc

    ok = dict(A=800, G=2400, BG=2, Qm=2, Nl=1)
    good = m._scr_array([(1, 0, 1)], 1)
    assert call([ok], [0], good, refused=False) == 0
    assert call([dict(ok, G=2 * 5 * 240, Nl=5)], [0], good) < 0 and "Nl above 4" in m.last_error()
    assert call([dict(ok, G=2 * 8 * 150, Nl=8)], [0], good) < 0 and "Nl above 4" in m.last_error()
    assert call([ok], [2], good) < 0 and "multiple of 4" in m.last_error()
    assert call([ok], [0], good, base=2) < 0 and "4-byte aligned" in m.last_error()
    assert call([ok], [0], None) < 0 and "scr is NULL" in m.last_error()
    for bad, reason in (((0x10000, 0, 0), "n_RNTI"), ((1, 0, 1024), "n_ID"), ((1, 2, 5), "q")):
        assert call([ok], [0], m._scr_array([bad], 1)) < 0 and reason in m.last_error()
    assert call([dict(ok, G=2401)], [0], good) < 0                        # G % (Qm Nl)
    assert call([ok], [0], good, mem=m.MEM_HOST | m.MEM_HARQ_DEVICE) < 0   # another mem value
    # a bad block behind a good one: nothing of the good one is written either
    assert call([ok, dict(ok, Nl=6, G=2 * 6 * 200)], [0, 4800], m._scr_array([(1, 0, 1), (2, 0, 2)], 2)) < 0
    # layer_mapping
    x = np.arange(48, dtype=np.int16)
    out = np.full(256, 0x5a5a, np.int16)

    def lm(n, Nl, stride, mem=m.MEM_HOST, src=x.ctypes.data, dst=out.ctypes.data):
        return Lq.nrLDPC_hip_layer_mapping(src, n, Nl, dst, stride, mem, None)

    for args, reason in (((24, 0, 24), "Nl"), ((24, 5, 24), "Nl"), ((24, 8, 24), "Nl"), ((23, 2, 12), "multiple of Nl"),
                         ((24, 2, 11), "layer_stride"), (((1 << 21) + 4, 4, 1 << 20), "2^21")):
        assert lm(*args) < 0 and reason in m.last_error(), args
    assert lm(24, 2, 12, mem=7) < 0 and "mem" in m.last_error()
    assert lm(24, 2, 12, src=None) < 0 and "null" in m.last_error()
    assert lm(24, 2, 12, dst=None) < 0 and "null" in m.last_error()
    assert lm(24, 2, 12, mem=m.MEM_DEVICE) < 0 and "device memory" in m.last_error()
    assert lm(24, 2, 12, dst=x.ctypes.data + 8) < 0 and "overlap" in m.last_error()
    assert (out == 0x5a5a).all() and np.array_equal(x, np.arange(48, dtype=np.int16))
    d_in = torch.zeros(48, dtype=torch.int16, device="cuda")
    d_out = torch.full((64,), 0x5a5a, dtype=torch.int16, device="cuda")
    assert lm(24, 2, 12, mem=m.MEM_DEVICE, src=d_in.data_ptr(), dst=out.ctypes.data) < 0 and "device memory" in m.last_error()
    assert lm(24, 3, 7, mem=m.MEM_DEVICE, src=d_in.data_ptr(), dst=d_out.data_ptr()) < 0
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0x5a5a).all()
    assert lm(0, 2, 0) == 0                                               # nothing to do
