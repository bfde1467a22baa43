"""-m gpu: the transport-block chain on the GPU against sch_np.py, the coding chain written from TS 38.212 alone, on the cases of
sch_cases.py (test_sch_model_host.py shows what they cover and which misreadings they would notice).  Every call but two goes
through the numpy host-memory entry points; the two device-resident ones move their arrays through page-locked tensors."""
import os
import time

import numpy as np
import pytest

import dl_slot_np as D
import sch_cases as SC
import sch_np as S
import test_dl_slot_host as H
from test_sch_model_host import blocks_of, model_bits, payload_of

pytestmark = pytest.mark.gpu
F32 = np.float32


def bits_at(case, rv):
    """the model's G bits of a case sent with another rv"""
    _, _, ds = blocks_of(case)
    seg, idx = S.positions(dict(case["tb"], rv=rv))
    return ds[seg, idx].astype(np.uint8)


def to_device(a):
    """a numpy array on the GPU by way of a page-locked tensor"""
    import torch
    h = torch.empty(a.shape, dtype=getattr(torch, str(a.dtype)), pin_memory=True)
    h.numpy()[...] = a
    d = h.cuda()
    torch.cuda.synchronize()
    return d


def to_host(d):
    import torch
    h = torch.empty(d.shape, dtype=d.dtype, pin_memory=True)
    h.copy_(d)
    torch.cuda.synchronize()
    return h.numpy().copy()


# ---- the way out -----------------------------------------------------------------------------------------------------------
def test_dlsch_encode_of_every_case_equals_the_model(hip):
    m = hip.ldpc
    tbs = [c["tb"] for c in SC.CASES]
    pays = [blocks_of(c)[0] for c in SC.CASES]
    t0 = time.perf_counter()
    coded = m.dlsch_encode_host(tbs, pays)
    t1 = time.perf_counter()
    for c, f in zip(SC.CASES, coded):
        assert f.size == c["tb"]["G"] and np.array_equal(f, model_bits(c)), c["id"]
    for c, p in zip(SC.CASES, pays):
        assert np.array_equal(m.dlsch_encode_host([c["tb"]], [p])[0], model_bits(c)), c["id"]
    print(f"{len(tbs)} blocks in one call {1e3 * (t1 - t0):.1f} ms, one by one {1e3 * (time.perf_counter() - t1):.1f} ms")


def test_dlsch_encode_device_resident_equals_the_model(hip):
    """the one device-resident call: PreparedTbBatch on the whole list"""
    import torch
    m = hip.ldpc
    tbs = [c["tb"] for c in SC.CASES]
    po, co, _, _ = m.tb_layout(tbs)
    pay = np.zeros(int(po[-1]) + 16, np.uint8)
    for i, c in enumerate(SC.CASES):
        pay[po[i]:po[i] + tbs[i]["A"] // 8] = blocks_of(c)[0]
    t0 = time.perf_counter()
    pay_d = to_device(pay)
    coded_d = torch.full((int(co[-1]) + 16,), 0x77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    m.PreparedTbBatch(tbs, pay_d, coded_d).encode()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    got = to_host(coded_d)
    print(f"torch set-up and upload {t1 - t0:.2f} s, the call and its synchronize {1e3 * (t2 - t1):.1f} ms, download {time.perf_counter() - t2:.2f} s")
    for i, c in enumerate(SC.CASES):
        assert np.array_equal(got[co[i]:co[i] + tbs[i]["G"]], model_bits(c)), c["id"]
        assert (got[co[i] + tbs[i]["G"]:co[i + 1]] == 0x77).all(), c["id"]


def test_blocks_outside_the_documented_contract_are_refused_with_its_message(hip):
    """E below the first filler, a circular buffer that ends before the fillers, one that ends inside them (sch_cases.REFUSED): both
    ways, before anything is enqueued"""
    m = hip.ldpc
    assert [tb["kind"] for tb in SC.REFUSED] == ["E below the first filler", "Ncb before the fillers", "Ncb inside the fillers"]
    for tb in SC.REFUSED:
        with pytest.raises(RuntimeError, match="nr_rate_matching: invalid parameters"):
            m.dlsch_encode_host([tb], [payload_of(tb)])
        harq = np.zeros((1, m.HARQ_STRIDE), np.int16)
        with pytest.raises(RuntimeError, match="nr_rate_matching_rx: invalid parameters"):
            m.ulsch_decode_host([dict(tb, round=0, llrLen=0)], [np.zeros(tb["G"], np.int16)], harq)


def symbol_subset():
    """one case per (Qm, Nl) pair the list holds"""
    seen, out = set(), []
    for c in SC.CASES:
        key = (c["tb"]["Qm"], c["tb"]["Nl"])
        if key not in seen and S.plan(c["tb"])["Zc"] <= 72:
            seen.add(key)
            out.append(c)
    assert len(out) == 16                                             # every Qm with every Nl
    return out


def table_points(d, Qm):
    """the model's closed-form points through the rule nr_qam.h documents for the table: (short)((float) level * 32768.f * s *
    0.70711f), float32 products left to right, truncated toward zero; level = the odd integer of the closed form"""
    root = np.sqrt(H.NORM[Qm])
    out = []
    for part in (d.real, d.imag):
        level = np.rint(part * root)
        assert np.abs(level - part * root).max() < 1e-9 and (level.astype(np.int64) % 2 == 1).all()
        v = level.astype(F32) * F32(32768.0)
        v = v * F32(H.C_QM[Qm])
        v = v * F32(0.70711)
        out.append(np.trunc(v).astype(np.int16))
    return np.stack(out, -1)


def test_scrambled_and_symbol_calls_equal_the_model_through_the_38211_model(hip):
    m = hip.ldpc
    cases = symbol_subset()
    rng = np.random.default_rng(8802)
    tbs = [c["tb"] for c in cases]
    pays = [blocks_of(c)[0] for c in cases]
    scr = [(int(rng.integers(1, 0xfff0)), int(rng.integers(0, 2)), int(rng.integers(0, 1024))) for _ in cases]
    words = m.dlsch_encode_scrambled_host(tbs, pays, scr)
    planes = m.dlsch_encode_symbols_host(tbs, pays, scr)
    for c, s, w, pl in zip(cases, scr, words, planes):
        tb = c["tb"]
        b = D.scramble(model_bits(c), *s)
        padded = np.concatenate([b, np.zeros((-b.size) % 32, np.uint8)])
        assert np.array_equal(w, np.packbits(padded, bitorder="little").view(np.uint32)), c["id"]
        lay = D.to_layers(D.modulate(b, tb["Qm"]), tb["Nl"])
        want = table_points(lay, tb["Qm"])
        assert pl.shape == want.shape and np.array_equal(pl, want), c["id"]


# ---- the way back ----------------------------------------------------------------------------------------------------------
def carries_the_block(p):
    """a first transmission at rv 0 that holds every systematic bit it can and at least six parity columns: the four core ones and
    two more.  Every case is one (asserted), which is why the payload is claimed for every case; nothing about the decoder went into
    this rule."""
    return min(p["E"]) >= p["fs"] + 6 * p["Zc"]


def check_buffers(cases, harq, rounds, llrs, what):
    row = 0
    for i, c in enumerate(cases):
        want = S.soft_buffers([r[i] for r in rounds], [l[i] for l in llrs])
        for r, b in enumerate(want):
            got = harq[row + r][:b.size]
            assert np.array_equal(got, b), (what, c["id"], r, np.flatnonzero(got != b)[:4])
        row += len(want)


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("kind", ["noiseless", "random"])
def test_ulsch_decode_soft_buffers_and_payloads_against_the_model(hip, fused, kind):
    """round 0 at rv 0 on buffers dirty over [0, Ncb), then from that state a second round at rv 1, at rv 2 and at rv 3.  After every call
    [0, Ncb) of every soft buffer is the model's plain sum.  Behind Ncb the buffers start at zero, as a caller's freshly allocated
    ones do: under LBRM a later round's rate mode reads positions there that no transmission reaches and only round 0's own mode
    clears (rules R0 / R1; test_gpu_tb_softbuf.py holds them), which is outside what 38.212 can say.
    Noiseless (+-8): the payload of every case comes back with ACK, after round 0 and after each second round.  Random LLRs in
    +-200: the soft buffers only."""
    m = hip.ldpc
    cases = SC.CASES
    rng = np.random.default_rng(31 + (kind == "random"))
    nseg = [S.plan(c["tb"])["C"] for c in cases]
    assert all(carries_the_block(S.plan(dict(c["tb"], rv=0))) for c in cases)

    def llr_of(rv):
        if kind == "random":
            return [rng.integers(-200, 201, c["tb"]["G"]).astype(np.int16) for c in cases]
        return [(8 * (1 - 2 * bits_at(c, rv).astype(np.int16))).astype(np.int16) for c in cases]

    def verdicts(out, ack, what):
        if kind == "noiseless":
            for c, o, a in zip(cases, out, ack):
                assert a and np.array_equal(o, blocks_of(c)[0]), (what, c["id"])

    prev = os.environ.get("NRLDPC_HIP_TB_FUSED")
    os.environ["NRLDPC_HIP_TB_FUSED"] = fused
    try:
        t0 = time.perf_counter()
        harq = np.zeros((sum(nseg), m.HARQ_STRIDE), np.int16)
        row = 0
        for c, n in zip(cases, nseg):
            harq[row:row + n, :S.plan(c["tb"])["Ncb"]] = rng.integers(-3000, 3000, (n, S.plan(c["tb"])["Ncb"]))
            row += n
        tbs0 = [dict(c["tb"], rv=0, round=0, llrLen=0) for c in cases]
        llr0 = llr_of(0)
        out, ack, _ = m.ulsch_decode_host(tbs0, llr0, harq, numMaxIter=8)
        verdicts(out, ack, "round 0")
        check_buffers(cases, harq, [tbs0], [llr0], (fused, kind, "round 0"))
        for rv in (1, 2, 3):
            again = harq.copy()
            tbs1 = [dict(t, rv=rv, round=1) for t in tbs0]
            llr1 = llr_of(rv)
            out, ack, _ = m.ulsch_decode_host(tbs1, llr1, again, numMaxIter=8)
            verdicts(out, ack, f"second round at rv {rv}")
            check_buffers(cases, again, [tbs0, tbs1], [llr0, llr1], (fused, kind, f"second round at rv {rv}"))
        print(f"fused {fused}, {kind}: {len(cases)} blocks, four calls and their checks {time.perf_counter() - t0:.2f} s")
    finally:
        if prev is None:
            os.environ.pop("NRLDPC_HIP_TB_FUSED", None)
        else:
            os.environ["NRLDPC_HIP_TB_FUSED"] = prev


# ---- the whole standard: payload -> 38.212 model -> 38.211 / 38.214 model -> grid ------------------------------------------
def whole_slot(m, name):
    """as test_dl_slot_host.build_slot, with the transport block sized and coded by sch_np instead of the oracle"""
    c = D.CASE_BY_NAME[name]
    rng = np.random.default_rng(9100 + int(name))
    ports = D.ports_of(c["ports"], c["Nl"])
    plane = H.plane_of(c["typ"], c["ncdm"], ports[0], c["pos"], c["start"], c["n_sym"], c["rb"])
    G = c["Qm"] * c["Nl"] * plane
    A = next(A for A, s in SC.contract_sizes(c["BG"], (G // 2 + 7) // 8 * 8, G))
    tb = dict(A=A, G=G, BG=c["BG"], Qm=c["Qm"], Nl=c["Nl"], rv=0, tbslbrm=0)
    scr = (int(rng.integers(1, 0xfff0)), 0, int(rng.integers(0, 1024)))
    pay = rng.integers(0, 256, A // 8, dtype=np.uint8)
    bits = S.dlsch(tb, pay)
    a = H.make_alloc(c, plane)
    segs, prgs = H.descriptors(m, c, a)
    p = dict(a, Qm=c["Qm"], rnti=scr[0], q=scr[1], n_id=scr[2])
    grid, mask = D.pdsch_grid(p, bits, c["n_tx"], beta_dmrs=1.0)
    want = c["amp"] / np.sqrt(2.0) * np.stack([grid.real, grid.imag], -1)
    return dict(case=c, tb=tb, scr=scr, pay=pay, segs=segs, model=grid, mask=mask, want=want, bound=H.bound_of(c, mask, []),
                stride=14 * c["N"] + H.TX_OFF + H.PAD, plane=plane)


def unprecoded(n_layers):
    return next(c["name"] for c in D.CASES if c["Nl"] == n_layers and c["prg"] is None and not c["si"])


@pytest.mark.parametrize("n_layers", [1, 2])
def test_payload_to_grid_against_both_models(hip, n_layers):
    import torch
    m = hip.ldpc
    sl = whole_slot(m, unprecoded(n_layers))
    c, tb = sl["case"], sl["tb"]
    po = m.tb_layout([tb])[0]
    co, total = m.tb_layout_symbols([tb])
    pay = np.zeros(int(po[-1]) + 16, np.uint8)
    pay[:tb["A"] // 8] = sl["pay"]
    pay_d = to_device(pay)
    lay_d = torch.zeros(total // 2 + 8, dtype=torch.int16, device="cuda")
    tx_d = torch.full(((c["n_tx"] + 1) * sl["stride"], 2), H.CANARY, dtype=torch.int16, device="cuda")
    m.dlsch_encode_symbols_device([tb], pay_d, lay_d, [sl["scr"]])
    m.pdsch_resource_mapping(lay_d, tx_d, sl["stride"], c["n_tx"], sl["segs"])
    torch.cuda.synchronize()
    got = to_host(tx_d).reshape(c["n_tx"] + 1, sl["stride"], 2)
    e_max = H.check_grid(sl, got, "GPU, both models")
    print(f"case {c['name']} ({n_layers} layers): error {e_max:.3f} / bound {float(sl['bound'].max()):.3f}")
