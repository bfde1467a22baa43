"""Scrambling inside the transport-block chain calls (nrLDPC_hip_dlsch_encode_scrambled / nrLDPC_hip_ulsch_decode_scrambled)
against their definition: the unscrambled chain call plus the separate (un)scrambling pass, every TB its own codeword."""
import os
import subprocess
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_tb_chain import make_tbs, valid_tbs
from test_scrambling_host import c_init_of, serial_gold, words_of

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent


def scrambled_words(bits, n_rnti, q, n_id):
    """numpy: bit k of word w = f(32w + k) ^ c(32w + k), zeros behind G"""
    G = bits.size
    nw = (G + 31) // 32
    b = np.zeros(nw * 32, np.uint8)
    b[:G] = (bits & 1) ^ serial_gold(c_init_of(n_rnti, q, n_id), G)
    return words_of(b)


def rand_scr(rng, n):
    return [(int(rng.integers(0, 0x10000)), int(rng.integers(0, 2)), int(rng.integers(0, 1024))) for _ in range(n)]


def encode_cases():
    big = dict(A=1277992, G=8 * 4 * 48000, BG=1, Qm=8, Nl=4, rv=0, tbslbrm=0)
    tiny = dict(A=24, G=2 * 40, BG=2, Qm=2, Nl=1, rv=0, tbslbrm=0)
    # 8 segments of E = 7404 / 7416 (not multiples of 32: every boundary word is shared), 2 layers
    odd = dict(A=valid_tbs(60000, 1), G=6 * 2 * 4937, BG=1, Qm=6, Nl=2, rv=1, tbslbrm=0)
    return make_tbs() + [big, tiny, odd]


def test_encode_scrambled_equals_encode_then_scrambling(hip):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(7311)
    tbs = encode_cases()
    scr = rand_scr(rng, len(tbs))
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
    bits = m.dlsch_encode_host(tbs, pays)
    want = [scrambled_words(f, *s) for f, s in zip(bits, scr)]
    # host buffers
    got = m.dlsch_encode_scrambled_host(tbs, pays, scr)
    for i in range(len(tbs)):
        assert np.array_equal(got[i], want[i]), i
    # device buffers, sentinels between the blocks' word ranges
    po, _, _, _ = m.tb_layout(tbs)
    co, total = m.tb_layout_packed(tbs)
    pay_h = np.zeros(int(po[-1]) + 16, np.uint8)
    for i, t in enumerate(tbs):
        pay_h[po[i]:po[i] + t["A"] // 8] = pays[i]
    coded = torch.full((total // 4 + 4,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    m.dlsch_encode_scrambled_device(tbs, torch.from_numpy(pay_h).cuda(), coded, scr)
    torch.cuda.synchronize()
    out = coded.cpu().numpy().view(np.uint32)
    mask = np.ones(out.size, bool)
    for i, t in enumerate(tbs):
        w0, nw = co[i] // 4, (t["G"] + 31) // 32
        assert np.array_equal(out[w0:w0 + nw], want[i]), i
        mask[w0:w0 + nw] = False
    assert (out[mask] == 0x5a5a5a5a).all()                              # nothing outside the blocks' words is written


@pytest.mark.parametrize("env", [{"NRLDPC_HIP_ENC_KERNEL": "bytes"}, {"NRLDPC_HIP_TB_TRUNC": "0"}])
def test_encode_scrambled_other_tx_paths(hip, env):
    if any(os.environ.get(k) == v for k, v in env.items()):
        pytest.skip("already this configuration")
    r = subprocess.run([sys.executable, "-m", "pytest", str(HERE / "test_gpu_tb_scrambled.py"), "-m", "gpu", "-q", "-x", "-k",
                        "test_encode_scrambled_equals_encode_then_scrambling"], env=dict(os.environ, **env), cwd=str(HERE.parent),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def noisy_llrs(rng, bits, sigma):
    x = np.clip(np.round((1 - 2 * bits.astype(np.float64)) * 8 + sigma * rng.standard_normal(bits.size)), -32768, 32767).astype(np.int16)
    k = rng.integers(0, bits.size, 3)
    x[k] = [-32768, 32767, 0]
    return x


def scramble_llrs(llr, n_rnti, q, n_id):
    """the transmitted signs: LLRs of the scrambled codeword (negation where c = 1; -(-32768) stays -32768)"""
    c = serial_gold(c_init_of(n_rnti, q, n_id), llr.size).astype(bool)
    out = llr.copy()
    out[c] = (-(llr[c].astype(np.int32))).astype(np.int16)
    return out


def decode_tbs():
    tbs = make_tbs()
    return [t for t in tbs if t["A"] < 60000]


@pytest.mark.parametrize("mode", ["device", "host", "pinned", "harq_device", "harq_library"])
def test_decode_scrambled_equals_unscramble_then_decode(hip, mode):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(zlib.crc32(mode.encode()))
    tbs = decode_tbs()
    n = len(tbs)
    scr = rand_scr(rng, n)
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
    po, co, ho, segs = m.tb_layout(tbs)
    llrlen_a, llrlen_b = [0] * n, [0] * n
    harq_a = np.zeros(int(ho[-1]) + 16, np.int16)
    harq_b = harq_a.copy()
    ids_a = [1000 + i for i in range(n)]
    ids_b = [2000 + i for i in range(n)]
    acks = []
    for rnd, (rv, sigma) in enumerate(((0, 10.0), (2, 3.0))):
        cur = [dict(t, rv=rv) for t in tbs]
        bits = m.dlsch_encode_host(cur, pays)
        llrs = [scramble_llrs(noisy_llrs(rng, f, sigma), *s) for f, s in zip(bits, scr)]
        llrs_copy = [x.copy() for x in llrs]
        rx_a = [dict(t, round=rnd, llrLen=llrlen_a[i]) for i, t in enumerate(cur)]
        rx_b = [dict(t, round=rnd, llrLen=llrlen_b[i]) for i, t in enumerate(cur)]
        # reference: the separate unscrambling pass, then the unscrambled call
        ref_llrs = [x.copy() for x in llrs]
        for x, (n_rnti, q, n_id) in zip(ref_llrs, scr):
            m.codeword_unscrambling(x, q, n_id, n_rnti)
        if mode == "device":
            def run(rx, L, harq, fn, **kw):
                llr_d = torch.zeros(int(co[-1]) + 16, dtype=torch.int16)
                for i, x in enumerate(L):
                    llr_d[co[i]:co[i] + x.size] = torch.from_numpy(x)
                llr_d = llr_d.cuda()
                before = llr_d.clone()
                h = torch.from_numpy(harq).cuda()
                pay = torch.zeros(int(po[-1]) + 16, dtype=torch.uint8, device="cuda")
                ack = torch.zeros(n, dtype=torch.uint8, device="cuda")
                itm = torch.zeros(n, dtype=torch.int32, device="cuda")
                fn(rx, llr_d, h, pay, ack, itm, **kw)
                torch.cuda.synchronize()
                assert torch.equal(llr_d, before)
                harq[:] = h.cpu().numpy()
                ph = pay.cpu().numpy()
                return [ph[po[i]:po[i] + t["A"] // 8] for i, t in enumerate(rx)], ack.cpu().numpy().astype(bool), itm.cpu().numpy()
            out_b = run(rx_b, ref_llrs, harq_b, m.ulsch_decode_device)
            out_a = run(rx_a, llrs, harq_a, m.ulsch_decode_scrambled_device, scrambling=scr)
        else:
            kw = dict(pinned=(mode == "pinned"))
            if mode == "harq_library":
                out_b = m.ulsch_decode_host(rx_b, ref_llrs, None, harq_ids=ids_b)
                out_a = m.ulsch_decode_scrambled_host(rx_a, llrs, None, scr, harq_ids=ids_a)
            elif mode == "harq_device":
                hb, ha = torch.from_numpy(harq_b).cuda(), torch.from_numpy(harq_a).cuda()
                out_b = m.ulsch_decode_host(rx_b, ref_llrs, hb)
                out_a = m.ulsch_decode_scrambled_host(rx_a, llrs, ha, scr)
                harq_b[:], harq_a[:] = hb.cpu().numpy(), ha.cpu().numpy()
            else:
                out_b = m.ulsch_decode_host(rx_b, ref_llrs, harq_b, **kw)
                out_a = m.ulsch_decode_scrambled_host(rx_a, llrs, harq_a, scr, **kw)
        for x, y in zip(llrs, llrs_copy):
            assert np.array_equal(x, y)                                   # the caller's LLRs are only read
        for i in range(n):
            assert np.array_equal(out_a[0][i], out_b[0][i]), (mode, rnd, i)
        assert np.array_equal(out_a[1], out_b[1]) and np.array_equal(out_a[2], out_b[2]), (mode, rnd)
        assert [t["llrLen"] for t in rx_a] == [t["llrLen"] for t in rx_b]
        if mode == "harq_library":
            # the circular buffer [0, Ncb) of every segment (behind it a pooled buffer keeps what an earlier user left)
            for i, t in enumerate(tbs):
                sg = O.segmentation(None, O.len_with_crc(1, t["A"]), t["BG"])
                N = (66 if t["BG"] == 1 else 50) * sg["Z"]
                Ncb = N if not t["tbslbrm"] else min(N, 3 * t["tbslbrm"] // (2 * sg["C"]))
                ha = m.harq_read(ids_a[i], segs[i] * m.HARQ_STRIDE).reshape(segs[i], m.HARQ_STRIDE)
                hb = m.harq_read(ids_b[i], segs[i] * m.HARQ_STRIDE).reshape(segs[i], m.HARQ_STRIDE)
                assert np.array_equal(ha[:, :Ncb], hb[:, :Ncb]), (rnd, i)
        else:
            assert np.array_equal(harq_a, harq_b), (mode, rnd)
        llrlen_a = [t["llrLen"] for t in rx_a]
        llrlen_b = [t["llrLen"] for t in rx_b]
        acks.append(out_a[1])
    if mode == "harq_library":
        m.harq_release()
    assert not acks[0].all() and acks[1].sum() > acks[0].sum()           # round 0 loses blocks, round 1 brings them back


@pytest.mark.parametrize("env", [{"NRLDPC_HIP_TB_FUSED": "0"}, {"NRLDPC_HIP_TB_MULTI": "2"}])
def test_decode_scrambled_other_rx_paths(hip, env):
    """the four-launch path, and small segments sharing workgroups (both through tb_rx_dematch_scr_kernel)"""
    if any(os.environ.get(k) == v for k, v in env.items()):
        pytest.skip("already this configuration")
    r = subprocess.run([sys.executable, "-m", "pytest", str(HERE / "test_gpu_tb_scrambled.py"), "-m", "gpu", "-q", "-x", "-k",
                        "test_decode_scrambled_equals_unscramble_then_decode or test_small_scrambled"], env=dict(os.environ, **env),
                       cwd=str(HERE.parent), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_small_scrambled_blocks_share_workgroups(hip):
    m = hip.ldpc
    rng = np.random.default_rng(99)
    tbs = []
    for A in (24, 104, 336, 808, 1544, 3104, 3824):
        for _ in range(4):
            Qm = int(rng.choice([2, 4, 6]))
            tbs.append(dict(A=A, G=max(int(A / 0.4) // Qm, 4) * Qm, BG=2, Qm=Qm, Nl=1, rv=0, tbslbrm=0))
    scr = rand_scr(rng, len(tbs))
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
    bits = m.dlsch_encode_host(tbs, pays)
    llrs = [scramble_llrs(noisy_llrs(rng, f, 4.0), *s) for f, s in zip(bits, scr)]
    ref = [x.copy() for x in llrs]
    for x, (n_rnti, q, n_id) in zip(ref, scr):
        m.codeword_unscrambling(x, q, n_id, n_rnti)
    harq_a = np.zeros((len(tbs), m.HARQ_STRIDE), np.int16)
    harq_b = harq_a.copy()
    rx_a = [dict(t, round=0, llrLen=0) for t in tbs]
    rx_b = [dict(t, round=0, llrLen=0) for t in tbs]
    a = m.ulsch_decode_scrambled_host(rx_a, llrs, harq_a, scr)
    b = m.ulsch_decode_host(rx_b, ref, harq_b)
    for i in range(len(tbs)):
        assert np.array_equal(a[0][i], b[0][i]), i
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(harq_a, harq_b)
    assert a[1].sum() > len(tbs) // 2


def test_decode_scrambled_sharded_over_logical_devices(hip, tmp_path):
    outs = []
    for devs in (None, "0,0,0"):
        env = dict(os.environ)
        env.pop("NRLDPC_HIP_DEVICES", None)
        if devs:
            env["NRLDPC_HIP_DEVICES"] = devs
        f = tmp_path / f"out_{devs or 'single'}.npz"
        r = subprocess.run([sys.executable, str(HERE / "multidev_scrambled_script.py"), str(f)], capture_output=True, text=True, env=env,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(np.load(f))
    a, b = outs
    assert sorted(a.files) == sorted(b.files) and len(a.files) >= 8
    for k in a.files:
        assert np.array_equal(a[k], b[k]), k
    assert a["ok"].all()


def test_slot_round_trip_64_blocks_on_device(hip):
    """The 64-TB slot (BASELINE configs[3]): encode with scrambling, a channel on the transmitted bits, decode with
    scrambling; every block ACKed with its payload, and the words equal the two-pass path's."""
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(64)
    t0 = dict(A=valid_tbs(213176, 1), G=(12 * 13 - 6) * 273 * 6, BG=1, Qm=6, Nl=1, rv=0, tbslbrm=0)
    tbs = [dict(t0) for _ in range(64)]
    scr = rand_scr(rng, 64)
    po, co_b, ho, segs = m.tb_layout(tbs)
    cw, total = m.tb_layout_packed(tbs)
    pay_h = rng.integers(0, 256, int(po[-1]) + 16, dtype=np.uint8)
    payload = torch.from_numpy(pay_h).cuda()
    words = torch.zeros(total // 4 + 4, dtype=torch.int32, device="cuda")
    m.dlsch_encode_scrambled_device(tbs, payload, words, scr)
    bytes_ = torch.zeros(int(co_b[-1]) + 16, dtype=torch.uint8, device="cuda")
    m.dlsch_encode_device(tbs, payload, bytes_)
    ref_words = torch.zeros_like(words)
    for i, (n_rnti, q, n_id) in enumerate(scr):
        m.codeword_scrambling(bytes_[co_b[i]:co_b[i] + t0["G"]], q, n_id, n_rnti, out=ref_words[cw[i] // 4:], size=t0["G"])
    torch.cuda.synchronize()
    assert torch.equal(words, ref_words)
    # channel on the transmitted (scrambled) bits: LLR = (1 - 2 bit) * 16 + noise
    w = words.cpu().numpy().view(np.uint32)
    llr_h = np.zeros(int(co_b[-1]) + 16, np.int16)
    for i in range(64):
        nw = (t0["G"] + 31) // 32
        tx = ((w[cw[i] // 4:cw[i] // 4 + nw, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)[:t0["G"]]
        llr_h[co_b[i]:co_b[i] + t0["G"]] = np.clip(np.round((1 - 2 * tx.astype(np.float64)) * 16 + 6 * rng.standard_normal(t0["G"])),
                                                    -128, 127).astype(np.int16)
    llr = torch.from_numpy(llr_h).cuda()
    harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
    pay_out = torch.zeros_like(payload)
    ack = torch.zeros(64, dtype=torch.uint8, device="cuda")
    itm = torch.zeros(64, dtype=torch.int32, device="cuda")
    rx = [dict(t, round=0, llrLen=0) for t in tbs]
    m.ulsch_decode_scrambled_device(rx, llr, harq, pay_out, ack, itm, scr)
    torch.cuda.synchronize()
    assert ack.cpu().numpy().all()
    out = pay_out.cpu().numpy()
    for i in range(64):
        assert np.array_equal(out[po[i]:po[i] + t0["A"] // 8], pay_h[po[i]:po[i] + t0["A"] // 8]), i



def test_scrambled_plans_and_graphs(hip):
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(5150)
    tbs = [dict(t, round=0, llrLen=0) for t in make_tbs()[:5]]
    scr = rand_scr(rng, len(tbs))
    po, co, ho, segs = m.tb_layout(tbs)
    cw, total = m.tb_layout_packed(tbs)
    pay_h = rng.integers(0, 256, int(po[-1]) + 16, dtype=np.uint8)
    payload = torch.from_numpy(pay_h).cuda()
    words = torch.zeros(total // 4 + 4, dtype=torch.int32, device="cuda")
    coded = torch.zeros(int(co[-1]) + 16, dtype=torch.uint8, device="cuda")
    # repeated calls, alternating scrambled / unscrambled on the same descriptors: each gives its own result
    ref = None
    for k in range(3):
        m.dlsch_encode_scrambled_device(tbs, payload, words, scr)
        m.dlsch_encode_device(tbs, payload, coded)
        torch.cuda.synchronize()
        ch = coded.cpu().numpy()
        for i, t in enumerate(tbs):
            assert np.array_equal(ch[co[i]:co[i] + t["G"]], O.dlsch_encode(t, pay_h[po[i]:po[i] + t["A"] // 8])), (k, i)
        if ref is None:
            ref = words.cpu().numpy().view(np.uint32).copy()
            for i, t in enumerate(tbs):
                assert np.array_equal(ref[cw[i] // 4:cw[i] // 4 + (t["G"] + 31) // 32], scrambled_words(ch[co[i]:co[i] + t["G"]], *scr[i]))
        assert np.array_equal(words.cpu().numpy().view(np.uint32), ref), k
    # one TB's RNTI changes: exactly that TB's words change
    scr2 = list(scr)
    scr2[2] = ((scr[2][0] + 1) & 0xffff, scr[2][1], scr[2][2])
    m.dlsch_encode_scrambled_device(tbs, payload, words, scr2)
    torch.cuda.synchronize()
    w2 = words.cpu().numpy().view(np.uint32)
    for i, t in enumerate(tbs):
        sl = slice(cw[i] // 4, cw[i] // 4 + (t["G"] + 31) // 32)
        assert np.array_equal(w2[sl], ref[sl]) == (i != 2), i
    # HIP graphs of both scrambled calls
    llr = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")
    harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
    pay_out = torch.zeros_like(payload)
    ack = torch.zeros(len(tbs), dtype=torch.uint8, device="cuda")
    itm = torch.zeros(len(tbs), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        enc = m.PreparedTbBatch(tbs, payload, words, scrambling=scr)
        dec = m.PreparedTbBatch(tbs, pay_out, llr, harq, ack, itm, scrambling=scr)
        for _ in range(3):
            enc.encode()
            dec.decode()
    torch.cuda.synchronize()
    g_enc, g_dec = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_enc, stream=side):
        enc.encode()
    with torch.cuda.graph(g_dec, stream=side):
        dec.decode()
    for rep in range(2):
        ph = rng.integers(0, 256, int(po[-1]) + 16, dtype=np.uint8)
        payload.copy_(torch.from_numpy(ph))
        words.zero_()
        g_enc.replay()
        torch.cuda.synchronize()
        wv = words.cpu().numpy().view(np.uint32)
        for i, t in enumerate(tbs):
            f = O.dlsch_encode(t, ph[po[i]:po[i] + t["A"] // 8])
            assert np.array_equal(wv[cw[i] // 4:cw[i] // 4 + (t["G"] + 31) // 32], scrambled_words(f, *scr[i])), (rep, i)
            tx = ((wv[cw[i] // 4:cw[i] // 4 + (t["G"] + 31) // 32, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)[:t["G"]]
            llr[co[i]:co[i] + t["G"]] = torch.from_numpy(((1 - 2 * tx.astype(np.int16)) * 20).astype(np.int16)).cuda()
        harq.zero_()
        g_dec.replay()
        torch.cuda.synchronize()
        assert ack.cpu().numpy().all(), rep
        out = pay_out.cpu().numpy()
        for i, t in enumerate(tbs):
            assert np.array_equal(out[po[i]:po[i] + t["A"] // 8], ph[po[i]:po[i] + t["A"] // 8]), (rep, i)


def test_scrambled_invalid_input(hip):
    import ctypes as C
    m = hip.ldpc
    L = m._tb_lib()
    tbs = [dict(A=800, G=2400, BG=2, Qm=2, Nl=1)]
    pay = np.zeros(128, np.uint8)
    for bad, reason in (((0x10000, 0, 0), "n_RNTI"), ((1, 0, 1024), "n_ID"), ((1, 2, 5), "q")):
        out = np.full(256, 0xA5A5A5A5, np.uint32)
        arr = m._tb_array(tbs, [0], [0], None)
        b = m.nrLDPC_hip_tb_batch_t(n_tb=1, tb=arr, payload=pay.ctypes.data, coded=out.ctypes.data, harq=None, harq_stride=0, ack=None,
                                    iter_max=None, mem=m.MEM_HOST, stream=None)
        assert L.nrLDPC_hip_dlsch_encode_scrambled(C.byref(b), m._scr_array([bad], 1)) < 0
        assert reason in m.last_error()
        assert (out == 0xA5A5A5A5).all()
        llr = np.ones(2400, np.int16)
        harq = np.full(m.HARQ_STRIDE, 7, np.int16)
        ack = np.full(1, 9, np.uint8)
        itm = np.full(1, 9, np.int32)
        arr = m._tb_array([dict(tbs[0], round=0)], [0], [0], [0])
        b = m.nrLDPC_hip_tb_batch_t(n_tb=1, tb=arr, payload=pay.ctypes.data, coded=llr.ctypes.data, harq=harq.ctypes.data,
                                    harq_stride=m.HARQ_STRIDE, ack=ack.ctypes.data, iter_max=itm.ctypes.data, mem=m.MEM_HOST, stream=None)
        assert L.nrLDPC_hip_ulsch_decode_scrambled(C.byref(b), m._scr_array([bad], 1)) < 0
        assert reason in m.last_error()
        assert (harq == 7).all() and ack[0] == 9 and itm[0] == 9 and (pay == 0).all()
    # NULL scr
    assert L.nrLDPC_hip_ulsch_decode_scrambled(C.byref(b), None) < 0 and "scr is NULL" in m.last_error()
    assert L.nrLDPC_hip_dlsch_encode_scrambled(C.byref(b), None) < 0 and "scr is NULL" in m.last_error()
    # misaligned coded_off
    out = np.full(256, 0xA5A5A5A5, np.uint32)
    arr = m._tb_array(tbs, [0], [2], None)
    b = m.nrLDPC_hip_tb_batch_t(n_tb=1, tb=arr, payload=pay.ctypes.data, coded=out.ctypes.data, harq=None, harq_stride=0, ack=None,
                                iter_max=None, mem=m.MEM_HOST, stream=None)
    assert L.nrLDPC_hip_dlsch_encode_scrambled(C.byref(b), m._scr_array([(1, 0, 1)], 1)) < 0
    assert "multiple of 4" in m.last_error() and (out == 0xA5A5A5A5).all()
