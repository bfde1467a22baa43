"""-m gpu: the soft-buffer positions at and beyond Ncb across HARQ rounds.

Nothing is ever received at positions >= Ncb, but the decoder reads up to np(R) = ncols(R) Zc - 2 Zc of them, and with
limited-buffer rate matching (Ncb < N) np(R) is usually larger than Ncb.  What those positions hold decides what a
retransmission decodes.  The rules pinned here:
  R0  on round 0 the positions [0, max(Ncb, np(R))) of every segment are zero before accumulation, R = the round's rate mode
      UNCUT, whatever NRLDPC_HIP_TB_TRUNC / _FUSED / _MULTI say and in every memory mode; nothing behind is written;
  R1  on rounds > 0 the buffer is used as it is, stale values beyond Ncb included (as in the reference);
  L   the library's buffers (MEM_HARQ_LIBRARY) that an id did not hold before the call read as zero wherever the call does
      not write: a new allocation, a buffer recycled from a released id, a regrow.
The caller's buffers are dirty EVERYWHERE at round 0; the oracle chain (tests/oracle_lib.py) starts from the same values with
R0 applied (tests/softbuf_np.py), and after every round every soft value of every whole row (HARQ_STRIDE), the ACK, the pass
count, the payload and llrLen must equal it."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as O
import softbuf_np as SB
from qam_np import demap_np
from test_gpu_tb_chain import valid_tbs
from test_gpu_qam import rx_symbols
from test_gpu_tb_scrambled import rand_scr, scramble_llrs

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
ROUNDS = ((0, 0), (1, 2), (2, 3), (3, 1))           # (round, rv)


def _mk(bits, G, BG, Qm, Nl, lbrm):
    return dict(A=valid_tbs(bits, BG), G=G, BG=BG, Qm=Qm, Nl=Nl, rv=0, tbslbrm=lbrm)


def lbrm_tbs():
    """both base graphs, C = 1 .. 8; the first six are limited-buffer blocks with Ncb < np(R0) (9000 < 23232, 6750 < 14784,
    4500 < 12800, ...), the high-rate ones (> 0.8) first transmissions the cut applies to"""
    return [
        _mk(30000, 54000, 1, 6, 1, 24000),    # BG1 C=4 Zc=352
        _mk(9600, 33600, 1, 8, 1, 9000),      # BG1 C=2 Zc=224, 256QAM
        _mk(5000, 14400, 2, 2, 1, 6000),      # BG2 C=2 Zc=256
        _mk(40000, 46800, 1, 6, 1, 30000),    # high rate, LBRM: E > Ncb (one lap and a bit), cut graph
        _mk(5000, 40000, 2, 4, 1, 6000),      # BG2 repetition: E = 20000 > Ncb = 4500
        _mk(60000, 72000, 1, 6, 2, 50000),    # high rate, LBRM, C=8, two layers
        _mk(3000, 3600, 2, 4, 1, 4000),       # high rate BG2 C=1, LBRM with Ncb > np(R0)
        _mk(20000, 24000, 1, 8, 1, 0),        # high rate, no LBRM (Ncb = N): the cut, nothing beyond Ncb
    ]


def segs_of(t):
    return O.segmentation(None, O.len_with_crc(1, t["A"]), t["BG"])["C"]


def _noisy(rng, f, sigma):
    return np.clip(np.round((1 - 2 * f.astype(np.float64)) * 8 + sigma * rng.standard_normal(f.size)), -200, 200).astype(np.int16)


def _sigma(t):
    return 3.0 if t["A"] / t["G"] > 0.8 else 7.0     # some blocks fail on round 0, some of those come back later


def _harq_buffers(m, mode, rows):
    if mode in ("host", "pinned"):
        return rows.copy()
    import torch
    return torch.from_numpy(rows.reshape(-1).copy()).cuda()


def _decode(m, mode, tbs, llrs, harq, kind="llr", scr=None):
    """one call of the chain in `mode`: (payloads, ack, iter_max, soft buffers as numpy rows).  kind: "llr" (plain LLRs),
    "scr" (scrambled LLRs) or "sym" (symbol records) -- the three entry points."""
    S = m.HARQ_STRIDE
    if mode != "device":
        fn = {"llr": m.ulsch_decode_host, "scr": m.ulsch_decode_scrambled_host, "sym": m.ulsch_decode_symbols_host}[kind]
        extra = () if kind == "llr" else (scr,)
        out, ack, itm = fn(tbs, llrs, harq, *extra, numMaxIter=8, pinned=mode == "pinned")
        rows = harq if isinstance(harq, np.ndarray) else harq.cpu().numpy().reshape(-1, S)
        return out, ack, itm, rows
    import torch
    po, co, _, _ = m.tb_layout(tbs)
    llr = torch.zeros(int(co[-1]) + 16, dtype=torch.int16, device="cuda")
    for i, x in enumerate(llrs):
        llr[int(co[i]):int(co[i]) + x.size] = torch.from_numpy(x).cuda()
    pay = torch.full((int(po[-1]) + 16,), 0x5a, dtype=torch.uint8, device="cuda")
    ack = torch.zeros(len(tbs), dtype=torch.uint8, device="cuda")
    itm = torch.zeros(len(tbs), dtype=torch.int32, device="cuda")
    if kind == "llr":
        m.ulsch_decode_device(tbs, llr, harq, pay, ack, itm, numMaxIter=8)
    elif kind == "scr":
        m.ulsch_decode_scrambled_device(tbs, llr, harq, pay, ack, itm, scr, numMaxIter=8)
    else:
        m.ulsch_decode_symbols_device(tbs, llr, harq, pay, ack, itm, scr, numMaxIter=8)
    torch.cuda.synchronize()
    p = pay.cpu().numpy()
    out = [p[int(po[i]):int(po[i]) + t["A"] // 8].copy() for i, t in enumerate(tbs)]
    return out, ack.cpu().numpy().astype(bool), itm.cpu().numpy(), harq.cpu().numpy().reshape(-1, S)


class OracleChain:
    """the reference's chain per block from the caller's round-0 buffers, with R0 applied on round 0"""

    def __init__(self, tbs, rows):
        self.segs = [segs_of(t) for t in tbs]
        first = np.cumsum([0] + self.segs)
        self.d = [[rows[first[i] + r].copy() for r in range(c)] for i, c in enumerate(self.segs)]
        self.state = [0] * len(tbs)

    def decode(self, i, t, llr, rnd):
        if rnd == 0:
            self.state[i] = 0
            SB.clear_first_round(t, self.d[i], 0)
        p, ack, its, self.state[i] = O.ulsch_decode(t, llr, self.d[i], 8, rnd, self.state[i], vec=True)
        return p, ack, its

    def check(self, tbs, got, what):
        out, ack, itm, rows = got
        row = 0
        for i, t in enumerate(tbs):
            assert t["llrLen"] == self.state[i], (what, i)
            for r in range(self.segs[i]):
                bad = np.flatnonzero(rows[row + r] != self.d[i][r])
                assert bad.size == 0, (what, i, r, "first differing soft-buffer positions", bad[:8].tolist(), SB.ncb_of(t))
            row += self.segs[i]


def _check_verdicts(what, i, t, got, ref, pays):
    out, ack, itm, _ = got
    p_ref, ack_ref, its = ref
    assert bool(ack[i]) == ack_ref and itm[i] == min(max(its), 9), (what, i, its, int(itm[i]))
    if ack_ref:
        assert np.array_equal(out[i], p_ref) and np.array_equal(out[i], pays[i]), (what, i)
    else:
        assert not out[i].any(), (what, i)                     # a lost block delivers zeros


def _rounds_on_dirty_buffers(m, mode, tbs, rng, kind="llr"):
    """the rounds of ROUNDS on caller buffers that are dirty everywhere; returns the ACKs per round"""
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
    scr = rand_scr(rng, len(tbs)) if kind != "llr" else None
    S = m.HARQ_STRIDE
    rows0 = rng.integers(-60, 60, (sum(segs_of(t) for t in tbs), S)).astype(np.int16)
    harq = _harq_buffers(m, mode, rows0)
    ref = OracleChain(tbs, rows0)
    acks = []
    for rnd, rv in ROUNDS:
        for t in tbs:
            t["rv"], t["round"] = rv, rnd
            if rnd == 0:
                t["llrLen"] = 0
        llrs, inputs = [], []
        for t, p, s in zip(tbs, pays, scr or [None] * len(tbs)):
            f = O.dlsch_encode(t, p)
            if kind == "sym":
                words = m.dlsch_encode_scrambled_host([t], [p], [s])[0]
                y, mags = rx_symbols(rng, words, t["G"], t["Qm"], _sigma(t) / 8.0, edges=False)
                inputs.append(m.pack_symbol_records([[y] + mags])[0])
                llrs.append(scramble_llrs(demap_np(y, mags, t["Qm"]), *s))   # oracle input: numpy demapping + unscrambling
            else:
                x = _noisy(rng, f, _sigma(t))
                llrs.append(x)
                inputs.append(scramble_llrs(x, *s) if kind == "scr" else x)
        got = _decode(m, mode, tbs, inputs, harq, kind, scr)
        for i, t in enumerate(tbs):
            _check_verdicts((mode, kind, rnd), i, t, got, ref.decode(i, t, llrs[i], rnd), pays)
        ref.check(tbs, got, (mode, kind, rnd))
        acks.append(got[1].copy())
    return acks


@pytest.mark.parametrize("mode", ["host", "pinned", "device", "harq_device"])
def test_dirty_caller_buffers_over_four_rounds(hip, mode):
    """Caller soft buffers that hold junk everywhere when round 0 starts (a HARQ process's d[r] reused for a new transport
    block): rv 0 -> 2 -> 3 -> 1.  Round 0 zeroes [0, max(Ncb, np(R0))) -- with LBRM 8 to 14 k positions per segment more
    than the reference's memset of Ncb -- and leaves the rest of the row alone; later rounds decode on whatever the rows
    hold.  Host rows (pageable or page-locked LLRs: staged downloads), device rows under host LLRs, all-device calls."""
    m = hip.ldpc
    tbs = lbrm_tbs()
    if os.environ.get("NRLDPC_HIP_TB_TRUNC") != "0":        # the blocks exercise what they are here for
        n_cut = n_beyond = 0
        for t in tbs:
            sg = O.segmentation(None, O.len_with_crc(1, t["A"]), t["BG"])
            E = O.get_E(t["G"], sg["C"], t["Qm"], t["Nl"], 0)
            R = O.get_R(0, E, t["BG"], sg["Z"], 0, 0)[0]
            cols = m.ulsch_decoder_columns(t["BG"], sg["Z"], sg["C"], sg["F"], sg["K"], t["tbslbrm"], 0, E, 0, R)
            ncb, np_full = SB.first_round_extents(t)[0][0]
            n_cut += cols < O.NCOLS[(t["BG"], R)]
            n_beyond += max(ncb, cols * sg["Z"] - 2 * sg["Z"]) < np_full      # the cut alone would clear less than R0
        assert n_cut >= 4 and n_beyond >= 2, (n_cut, n_beyond)
    acks = _rounds_on_dirty_buffers(m, mode, tbs, np.random.default_rng(2026))
    assert 0 < acks[0].sum() < len(tbs), acks[0]
    assert any(a[i] and not acks[0][i] for a in acks[1:] for i in range(len(tbs))), acks   # combining brings blocks back


@pytest.mark.parametrize("env", [{"NRLDPC_HIP_TB_TRUNC": "0"}, {"NRLDPC_HIP_TB_FUSED": "0"}, {"NRLDPC_HIP_TB_MULTI": "2"}])
def test_dirty_caller_buffers_other_rx_paths(hip, env):
    """R0 does not depend on the performance switches: the whole-mode first transmissions, the four-launch path, shared
    decoder workgroups (a child pytest with the variable in its environment)"""
    if any(os.environ.get(k) == v for k, v in env.items()):
        pytest.skip("already this configuration")
    r = subprocess.run([sys.executable, "-m", "pytest", str(HERE / "test_gpu_tb_softbuf.py"), "-m", "gpu", "-q", "-x", "-k",
                        "test_dirty_caller_buffers_over_four_rounds"], env=dict(os.environ, **env), cwd=str(HERE.parent),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("kind,mode", [("scr", "host"), ("scr", "device"), ("sym", "host"), ("sym", "device")])
def test_dirty_buffers_through_the_scrambled_and_symbol_calls(hip, kind, mode):
    """the same round sequence through nrLDPC_hip_ulsch_decode_scrambled and _symbols (host and device memory) on limited-
    buffer blocks; the oracle's LLRs come from numpy demapping (qam_np.demap_np) and unscrambling"""
    m = hip.ldpc
    tbs = [t for t in lbrm_tbs() if t["tbslbrm"]][:5]
    acks = _rounds_on_dirty_buffers(m, mode, tbs, np.random.default_rng(77 + len(kind + mode)), kind)
    assert acks[-1].sum() > 0


def test_library_buffers_read_zero_where_a_call_does_not_write(hip):
    """Rule L.  Id X decodes a large block (12 segments, no LBRM: rows written up to N) over two rounds and is released;
    new ids whose size the pool serves with X's buffers (a pooled buffer goes to a request of n within [n, 2n]) then take
    limited-buffer blocks and blocks of a smaller Zc over two rounds; one id regrows to a larger block on round 0; all again
    after harq_release_all.  harq_read of every whole row equals the oracle chain started from zeros."""
    m = hip.ldpc
    S = m.HARQ_STRIDE
    rng = np.random.default_rng(4711)
    m.harq_release()

    def run(tbs, ids, rounds):
        pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
        ref = OracleChain(tbs, np.zeros((sum(segs_of(t) for t in tbs), S), np.int16))
        acks = []
        for rnd, rv in rounds:
            llrs = []
            for t, p in zip(tbs, pays):
                t["rv"], t["round"] = rv, rnd
                if rnd == 0:
                    t["llrLen"] = 0
                llrs.append(_noisy(rng, O.dlsch_encode(t, p), _sigma(t)))
            out, ack, itm = m.ulsch_decode_host(tbs, llrs, None, numMaxIter=8, harq_ids=ids)
            rows = np.concatenate([m.harq_read(h, segs_of(t) * S).reshape(-1, S) for h, t in zip(ids, tbs)])
            got = (out, ack, itm, rows)
            for i, t in enumerate(tbs):
                _check_verdicts(("library", ids[i], rnd), i, t, got, ref.decode(i, t, llrs[i], rnd), pays)
            ref.check(tbs, got, ("library", ids, rnd))
            acks.append(ack.copy())
        return acks

    X = 0x7000
    big = [_mk(100000, 8 * 4 * 9000, 1, 8, 4, 0)]
    assert segs_of(big[0]) == 12
    run(big, [X], ((0, 0), (1, 2)))
    assert (m.harq_read(X, 12 * S).reshape(12, S)[:, :66 * 384] != 0).mean() > 0.9     # X's rows are written throughout
    assert m.harq_release(X) == 0

    def new_ids_stage(base, order):
        small = [_mk(60000, 72000, 1, 6, 2, 50000),                 # C=8, LBRM: 8 * S within [12 S / 2, 12 S]: X's buffer
                 _mk(45000, 60000, 1, 4, 1, 0),                     # C=6, Zc=352 < 384, no LBRM
                 _mk(20000, 60000, 2, 4, 1, 0),                     # BG2, C=6, no LBRM
                 _mk(30000, 54000, 1, 6, 1, 24000)]                 # C=4, LBRM (a new allocation or a smaller pooled one)
        assert [segs_of(t) for t in small] == [8, 6, 6, 4]
        for k in order:                                             # one id at a time: each takes what the pool has then
            run([small[k]], [base + k], ((0, 0), (1, 2)))
        # regrow on round 0: the id of the C=4 block takes a C=8 block
        run([_mk(60000, 72000, 1, 6, 2, 50000)], [base + 3], ((0, 0), (1, 3)))

    new_ids_stage(0x7100, (0, 1, 2, 3))                             # the C=8 block gets X's buffer
    assert m.harq_release() == 0
    new_ids_stage(0x7200, (3, 2, 1, 0))                             # every buffer comes from the pool, most of another kind of block
    m.harq_release()
