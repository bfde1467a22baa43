"""-m gpu: the documented NRLDPC_HIP_* switches that select other device code or another data path, each in a fresh process.

The library caches code entries and reads most switches once per process, so a setting needs a child: test_switch_set starts
`pytest <this file> -m gpu -k <probes>` with the set's environment.  The PROBES below are ordinary gpu tests -- small, checked
bit-exact against the oracle (output bytes, pass counts, ACKs, soft buffers) -- that also run in this process in the default
configuration, where they are the control and where their run time sizes the children's time limits.

SWITCHES lists every switch the library reads or INTEGRATION section 3c documents: probed here, or exempt with a reason
(tests/test_switches_host.py checks the list against the sources).  The schedule knobs' values and the codes each of them acts
on come from tests/switch_knobs.py, which compares the table builder's descriptors on the CPU.

Evidence that a set took effect is what the library reports by itself:
  code_info   nrLDPC_hip_code_info: workgroup size / LDS bytes / check-node tasks differ from the parent's default reading and
              equal what the table builder gives under the set (FAST_WAVES, EXT_GLOBAL, CN_DOUBLE, PAIR19)
  stderr      the library's own diagnostics (SRV_DEBUG: where the mailboxes live; DEBUG_SYNC: the stages, chunk by chunk)
  inside a probe: nrLDPC_hip_server_stats (status, calls served), kernel 5 refused under MULTI=0, a caller's predicate never
              called under CRC_TRUST_POINTER=1
For BN_SHORT, BN_GROUP (descriptor differences only: switch_knobs.affected_codes, same ldpc_graph.c) and for FAIR, TB_FAIR, TB_PRIO,
TB_LROW, TB_OVERLAP, TB_STAGGER_US, PULL_STAGGER_US, HOST_PULL, HOST_CHUNK, TB_PULL, TB_PULL_MAX_MB, TB_HOST_CHUNKS, TB_CRC_CHUNK,
BOUNCE_THREADS, CUT, MULTI=<n>, ENC_THREADS, ENC_SLOTS the library reports nothing: the evidence is the name guard alone.
(nrLDPC_hip_ulsch_decoder_columns, which reports a cut, is about the transport-block chain's and follows TB_TRUNC; NRLDPC_HIP_CUT,
the per-segment entry point's, shows in no report.)
A knob value under which the table builder gives a workgroup shape up (switch_knobs.FALLS_BACK: BN_SHORT=30 on BG1 Zc = 384 R = 1/3)
is a "falls back, same results" case: code_info names the generic kernel, kernels 3 / 4 are refused by name, and the batch, host-batch
and per-segment probes get the oracle's results from the generic kernel."""
import ctypes as C
import functools
import json
import os
import re
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as O
import switch_knobs as K
from common import kbits, make_llr, random_info

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
EXPECT_ENV = "SWITCH_SET_EXPECT"        # parent -> child: the set's id, the parent's default code_info, the evidence to show

PROBES = {"decoder_batch": "test_probe_decoder_batch", "host_batch": "test_probe_host_batch",
          "segment_call": "test_probe_segment_call", "ul_chain": "test_probe_ul_chain", "dl_chain": "test_probe_dl_chain"}

_OWNED = "run by an existing test: "
SWITCHES = {
    # the fast decoder's schedule knobs
    "FAST_WAVES": ("probe", "decoder_batch"), "EXT_GLOBAL": ("probe", "decoder_batch"), "BN_SHORT": ("probe", "decoder_batch,segment_call"),
    "BN_GROUP": ("probe", "decoder_batch,segment_call"), "CN_DOUBLE": ("probe", "decoder_batch,segment_call"),
    "PAIR19": ("probe", "decoder_batch,segment_call"),
    # fallbacks the library picks by itself on other machines or call sizes
    "SRV_BAR": ("probe", "segment_call"), "HOST_PULL": ("probe", "host_batch"), "HOST_CHUNK": ("probe", "host_batch"),
    "TB_PULL": ("probe", "ul_chain"), "TB_PULL_MAX_MB": ("probe", "ul_chain"), "TB_HOST_CHUNKS": ("probe", "ul_chain"),
    "TB_LROW": ("probe", "ul_chain"), "CUT": ("probe", "segment_call"), "MULTI": ("probe", "decoder_batch,host_batch"),
    "TB_CRC_CHUNK": ("probe", "dl_chain"), "BOUNCE_THREADS": ("probe", "ul_chain"),
    # scheduling switches with kernel code behind them
    "FAIR": ("probe", "decoder_batch"), "TB_FAIR": ("probe", "ul_chain"), "TB_PRIO": ("probe", "ul_chain"),
    "TB_OVERLAP": ("probe", "ul_chain"), "TB_STAGGER_US": ("probe", "ul_chain"), "PULL_STAGGER_US": ("probe", "decoder_batch"),
    # further switches with a code path of their own
    "ENC_THREADS": ("probe", "dl_chain"), "ENC_SLOTS": ("probe", "dl_chain"), "CRC_TRUST_POINTER": ("probe", "segment_call"),
    "SRV_DEBUG": ("probe", "segment_call"), "DEBUG_SYNC": ("probe", "ul_chain"),
    # exemptions
    "TB_FUSED": ("exempt", _OWNED + "test_gpu_tb_chain, test_gpu_tb_softbuf, test_gpu_tb_resident"),
    "TB_TRUNC": ("exempt", _OWNED + "test_gpu_tb_softbuf::test_dirty_caller_buffers_other_rx_paths"),
    "TB_MULTI": ("exempt", _OWNED + "test_gpu_tb_chain::test_small_transport_blocks_share_workgroups"),
    "TB_FILL": ("exempt", _OWNED + "test_gpu_tb_chain::test_small_transport_blocks_share_workgroups"),
    "TB_CLASSES": ("exempt", _OWNED + "test_gpu_tb_chain::test_small_transport_blocks_share_workgroups"),
    "TB_ABORT": ("exempt", _OWNED + "test_gpu_tb_chain::test_abort_stops_the_siblings_of_a_failed_segment"),
    "ENC_KERNEL": ("exempt", _OWNED + "test_gpu_encoder, test_gpu_tb_chain::test_unfused_tx_path_too"),
    "ENC_SERVER": ("exempt", _OWNED + "test_gpu_encoder"),
    "ZC": ("exempt", _OWNED + "test_gpu_decoder (the general kernels against the per-Zc instantiations)"),
    "SERVER": ("exempt", _OWNED + "test_gpu_decoder"), "SRV_WAIT": ("exempt", _OWNED + "test_gpu_decoder"),
    "SRV_SLOTS": ("exempt", _OWNED + "test_gpu_decoder"), "SRV_IDLE_US": ("exempt", _OWNED + "test_gpu_decoder"),
    "REQUIRE_BUILD": ("exempt", _OWNED + "test_abi"),
    "SRV_TEST_FAIL_LAUNCH": ("exempt", "test hook, owned by the resident server's launch-failure test (tests/abi_threads.c)"),
    "TEST_STAGE_HARQ": ("exempt", "test hook, owned by test_gpu_tb_resident"),
    "DEVICES": ("exempt", "multi-GPU: the multidev_* scripts"), "DEVICE": ("exempt", "multi-GPU: the ordinal of the one GPU used"),
    "DEC_TRACE": ("exempt", "diagnostics: writes a trace file"), "TB_TRACE": ("exempt", "diagnostics: writes a trace file"),
    "ENC_STOP": ("exempt", "profiling aid, only compiled into builds with -DENC_PHASE_STOP"),
    "PAGEABLE_DIRECT": ("exempt", "diagnostics: control arm of a soak, the arrangement the bounce policy replaced because it faulted"),
    "T2_LIB": ("exempt", "Python mirror only: which library file to load"), "LIB": ("exempt", "Python mirror only: which library file to load"),
}


def _env(**kw):
    return {K.PREFIX + k: str(v) for k, v in kw.items()}


# evidence: ("code_info", field, (BG, Zc, R)) -- a code on which a knob of the set moves that field of nrLDPC_hip_code_info;
# ("falls_back", "fast", code) -- nrLDPC_hip_code_info names the generic kernel for a code the fast kernel serves by default;
# ("stderr", text) / ("stderr_re", pattern) -- a line of the library's own diagnostics
SWITCH_SETS = [
    dict(id="waves5", env=_env(FAST_WAVES=5, BN_SHORT=0, CN_DOUBLE=0, FAIR=0, HOST_PULL=0, HOST_CHUNK=16, MULTI=0),
         probes=("decoder_batch", "host_batch"),
         evidence=[("code_info", "threads", (1, 384, 13)), ("code_info", "cn_tasks", (2, 384, 15))]),
    dict(id="combined", env=dict(K.full_env(K.KNOB_VALUES["combined"]), **_env(TB_LROW=0, TB_FAIR=0, TB_PRIO=0)),
         probes=("decoder_batch", "segment_call", "ul_chain"),
         evidence=[("code_info", "threads", (1, 384, 13)), ("code_info", "lds_bytes", (2, 208, 13)), ("code_info", "cn_tasks", (1, 384, 89)),
                   ("code_info", "cn_tasks", (2, 384, 15))]),
    # BN_SHORT=30: the fall-back value (switch_knobs.FALLS_BACK) -- every probe the table names for BN_SHORT runs under it
    dict(id="waves9", env=_env(FAST_WAVES=9, BN_SHORT=30, BN_GROUP=1, CN_DOUBLE=4, HOST_CHUNK=7, PULL_STAGGER_US=0, MULTI=3),
         probes=("decoder_batch", "host_batch", "segment_call"),
         evidence=[("code_info", "threads", (1, 384, 23)), ("code_info", "cn_tasks", (2, 384, 15)), ("falls_back", "fast", (1, 384, 13))]),
    dict(id="waves13", env=_env(FAST_WAVES=13, EXT_GLOBAL=0, BN_GROUP=5, SRV_BAR=0, SRV_DEBUG=1, CUT=0),
         probes=("decoder_batch", "segment_call"),
         evidence=[("code_info", "threads", (1, 384, 13)), ("code_info", "lds_bytes", (1, 384, 23)),
                   ("stderr", "decoder server: 64 slots, requests pulled from host memory")]),
    dict(id="waves1", env=_env(FAST_WAVES=1, EXT_GLOBAL=1, BN_GROUP=2, CRC_TRUST_POINTER=1), probes=("decoder_batch", "segment_call"),
         evidence=[("code_info", "threads", (1, 384, 13)), ("code_info", "lds_bytes", (2, 384, 15))]),
    dict(id="waves2", env=_env(FAST_WAVES=2, BN_SHORT=3, TB_PULL=0, TB_HOST_CHUNKS=3, BOUNCE_THREADS=0, TB_OVERLAP=1, TB_STAGGER_US=20),
         probes=("decoder_batch", "ul_chain"), evidence=[("code_info", "threads", (1, 384, 13))]),
    dict(id="waves3", env=_env(FAST_WAVES=3, CN_DOUBLE=3, TB_PULL_MAX_MB=0, TB_HOST_CHUNKS=2, TB_PRIO=3, DEBUG_SYNC=1, TB_CRC_CHUNK=1),
         probes=("decoder_batch", "ul_chain", "dl_chain"),
         evidence=[("code_info", "threads", (1, 384, 13)), ("code_info", "cn_tasks", (2, 384, 15)),
                   ("stderr_re", r"\[tb_rx dbg\] ok: [^\n]* \(tb0 [1-6] ntb [1-6] staged 1\)")]),      # a chunk that does not start at block 0
    dict(id="waves7", env=_env(FAST_WAVES=7, PAIR19=0, TB_CRC_CHUNK=2, ENC_THREADS=128, ENC_SLOTS=3), probes=("decoder_batch", "dl_chain"),
         evidence=[("code_info", "threads", (1, 384, 13)), ("code_info", "cn_tasks", (1, 384, 89))]),
    dict(id="waves16", env=_env(FAST_WAVES=16), probes=("decoder_batch",), evidence=[("code_info", "threads", (1, 384, 23))]),
]

INFO_INDEX = {"threads": 4, "lds_bytes": 5, "cn_tasks": 6}      # nrLDPC_hip_code_info (of the fast kernel, where it serves the code)


def code_info_raw(m, BG, Z, R):
    L = m.load_library()
    a = (C.c_int32 * 8)()
    L.nrLDPC_hip_code_info.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]
    assert L.nrLDPC_hip_code_info(BG, Z, R, a) == 0
    return dict({k: int(a[i]) for k, i in INFO_INDEX.items()}, fast=int(a[3]))


def _given_up(BG, Z, R):
    """under this process' knobs the table builder gives a workgroup shape of the code up (switch_knobs.FALLS_BACK): the library then
    serves the code with the generic kernel, whatever the call"""
    return not (K.fast_info(BG, Z, R, "throughput")["f_ok"] and K.fast_info(BG, Z, R, "latency")["f_ok"])


def _own_knobs():
    """the schedule knobs this process runs under (names without the prefix)"""
    return {k: os.environ[K.PREFIX + k] for k in K.KNOBS if K.PREFIX + k in os.environ}


def _probe_codes():
    """the codes a decoder probe runs: in the default configuration the whole list; under knobs the codes whose throughput-shape
    descriptor one of those knob values changes"""
    own = _own_knobs()
    if not own:
        return list(K.CODES)
    labels = [lab for lab, short in K.KNOB_VALUES.items() if set(short.items()) <= set(own.items())]
    codes = K.affected_throughput_codes(labels)
    assert labels and codes, own
    return codes


def _n_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- control timing: how long each probe takes in this process ---------------------------------------------------------------------
_CONTROL_SECONDS = {}


@pytest.fixture(autouse=True)
def _time_probes(request):
    t0 = time.perf_counter()
    yield
    if request.node.name.startswith("test_probe_"):
        _CONTROL_SECONDS[request.node.name] = time.perf_counter() - t0


# ---- probes ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _decoder_inputs(BG, Z, R):
    """8 distinct inputs of a code -- noisy code words from hopeless to easy, uniform int8 -- and the oracle's results for caps 1
    and 8 (computed once per process)"""
    rng = np.random.default_rng(1000 * BG + 10 * Z + R)
    info = random_info(rng, BG, Z, with_crc24b=True)
    llrs = [make_llr(rng, BG, Z, R, k, info) for k in (-3.0, -1.0, -0.3, 0.3, 1.0, 2.0, 4.0)] + [make_llr(rng, BG, Z, R, "rand")]
    refs = {cap: [O.decode(BG, Z, R, x, cap, 0, out_init=0x33) for x in llrs] for cap in (1, 8)}
    return np.stack(llrs), refs


def _check_cycled(what, it, out, refs):
    it, out = np.asarray(it), np.asarray(out)
    for j, (n_ref, out_ref) in enumerate(refs):
        assert (it[j::len(refs)] == n_ref).all(), (what, j, n_ref, it[j::len(refs)][:8].tolist())
        rows = out[j::len(refs), :out_ref.size]
        bad = np.flatnonzero((rows != out_ref[None, :]).any(axis=1))
        assert bad.size == 0, (what, j, "blocks", (bad[:8] * len(refs) + j).tolist())


def test_probe_decoder_batch(hip):
    """LDPCdecoder_batch on the codes the process' knobs act on: one batch of a little more than a full round of workgroups (so that
    a second round starts and, where the shape has two or more workgroups of at least 256 threads per CU, the `fair` turns run),
    8 distinct inputs cycled, kernels 3 and 4 (5 where it serves the code), caps 1 and 8, device buffers; the automatic choice on
    page-locked host buffers (the pull kernel, with its first-round stagger on the codes that fill a CU with one workgroup); the
    three output modes once."""
    import torch
    m = hip.ldpc
    n_cus = _n_cus()
    multi_off = os.environ.get(K.PREFIX + "MULTI") == "0"
    fair_seen = staggered = fell_back = 0
    codes = _probe_codes()
    for ci, (BG, Z, R) in enumerate(codes):
        llrs, refs = _decoder_inputs(BG, Z, R)
        fi = K.fast_info(BG, Z, R)                       # the builder under this process' own environment
        info = code_info_raw(m, BG, Z, R)
        gave_up = _given_up(BG, Z, R)
        assert info["fast"] == (0 if gave_up else 1) and (gave_up or info["threads"] == fi["threads"]), (BG, Z, R, fi, info)
        fell_back += gave_up
        n = n_cus * (1 if gave_up else fi["wg_per_cu"]) + 3
        fair_seen += (not gave_up) and fi["wg_per_cu"] >= 2 and fi["threads"] >= 256
        batch = np.ascontiguousarray(llrs[np.arange(n) % 8])
        stride = (m.out_bytes(BG, Z, R, 0) + 3) // 4 * 4
        d_llr = torch.from_numpy(batch).cuda()
        # a code the fast section is off for: the fast kernel is refused by name, the generic kernel and the automatic choice serve
        kernels = (3, 4, 0, 1) if gave_up else (3, 4, 5) if 8 <= Z <= 64 else (3, 4)
        for kern in kernels:
            for cap in (1, 8):
                d_out = torch.full((n, stride), 0x33, dtype=torch.uint8, device="cuda")
                d_it = torch.zeros(n, dtype=torch.int32, device="cuda")
                refused = "no multi-block variant" if kern == 5 and multi_off else "fast kernel not applicable" if gave_up and kern >= 2 else None
                if refused:                              # (MULTI=0: there is no multi-block variant, and the library says so)
                    with pytest.raises(RuntimeError, match=refused):
                        m.decode_batch_device(BG, Z, R, d_llr, d_out, d_it, numMaxIter=cap, kernel=kern)
                    continue
                m.decode_batch_device(BG, Z, R, d_llr, d_out, d_it, numMaxIter=cap, kernel=kern)
                torch.cuda.synchronize()
                _check_cycled((BG, Z, R, "device", kern, cap), d_it.cpu().numpy(), d_out.cpu().numpy(), refs[cap])
        # host buffers, page-locked: the decoder's workgroups pull their rows over the link
        keep = m.PinnedArray(batch.shape, np.int8)
        keep.a[:] = batch
        it, out = m.decode_batch_host(BG, Z, R, keep.a, numMaxIter=8, out=np.full((n, stride), 0x33, np.uint8))
        _check_cycled((BG, Z, R, "pinned host"), it, out, refs[8])
        staggered += (not gave_up) and fi["wg_per_cu"] == 1
        if ci == 0:
            for mode in (1, 2):
                ob = m.out_bytes(BG, Z, R, mode)
                d_out = torch.full((n, (ob + 3) // 4 * 4), 0x33, dtype=torch.uint8, device="cuda")
                d_it = torch.zeros(n, dtype=torch.int32, device="cuda")
                m.decode_batch_device(BG, Z, R, d_llr, d_out, d_it, numMaxIter=8, outMode=mode, kernel=1 if gave_up else 3)
                torch.cuda.synchronize()
                _check_cycled((BG, Z, R, "mode", mode), d_it.cpu().numpy(), d_out.cpu().numpy(),
                              [O.decode(BG, Z, R, x, 8, mode, out_init=0x33) for x in llrs])
    own = _own_knobs()
    if not own:
        assert fair_seen >= 3 and staggered >= 2 and fell_back == 0, (fair_seen, staggered, fell_back)
    if K.PREFIX + "FAIR" in os.environ:                  # the switch is turned on launches that would take the turns without it
        assert fair_seen >= 1, fair_seen
    want = {f[1] for f in K.FALLS_BACK if set(K.KNOB_VALUES[f[0]].items()) <= set(own.items())}
    assert fell_back == len(want & set(codes)) == len(want), (fell_back, want)


def test_probe_host_batch(hip):
    """Host-buffer batches of 40 blocks (at least the 16 the pull path asks for, no multiple of a forced chunk): pageable and
    page-locked LLRs, a fast-kernel code and one only the generic kernel (and the interleaved multi-block variant) serves."""
    m = hip.ldpc
    multi_off = os.environ.get(K.PREFIX + "MULTI") == "0"
    for BG, Z, R in ((1, 352, 23), (2, 7, 13)):
        rng = np.random.default_rng(40 + Z)
        llrs = [make_llr(rng, BG, Z, R, k) for k in (-2.0, -0.5, 0.5, 2.0, "rand")]
        batch = np.ascontiguousarray(np.stack(llrs)[np.arange(40) % 5])
        stride = (m.out_bytes(BG, Z, R, 0) + 3) // 4 * 4
        for cap in (1, 8):
            refs = [O.decode(BG, Z, R, x, cap, 0, out_init=0x33) for x in llrs]
            keep = m.PinnedArray(batch.shape, np.int8)
            keep.a[:] = batch
            for what, arr in (("pageable", batch), ("pinned", keep.a)):
                for kern in (0, 5) if Z == 7 else (0,):
                    pre = np.full((40, stride), 0x33, np.uint8)
                    if kern == 5 and multi_off:
                        with pytest.raises(RuntimeError, match="no multi-block variant"):
                            m.decode_batch_host(BG, Z, R, arr, numMaxIter=cap, out=pre, kernel=kern)
                        continue
                    it, out = m.decode_batch_host(BG, Z, R, arr, numMaxIter=cap, out=pre, kernel=kern)
                    _check_cycled((BG, Z, R, what, kern, cap), it, out, refs)


def test_probe_segment_call(hip):
    """LDPCdecoder(), the per-segment entry point, with the library's nrLDPC_hip_check_crc: with and without an all-zero tail
    (served on the cut graph unless CUT=0), through the resident server (its statistics count the calls); once with a caller's own
    predicate, which is called on the host -- or, under CRC_TRUST_POINTER=1, never.  A code the fast section is off for
    (switch_knobs.FALLS_BACK) is among the codes: the server then runs its generic body, same results.  (Whether CUT=0 took effect
    does not show here -- results are equal by design -- nor anywhere else: nrLDPC_hip_ulsch_decoder_columns reports the chain's cut,
    which TB_TRUNC steers, not this one.)"""
    m = hip.ldpc
    before = m.server_stats()
    assert before["status"] == 0, before
    trust = os.environ.get(K.PREFIX + "CRC_TRUST_POINTER") == "1"
    n_calls = 0
    for BG, Z, R in ((1, 384, 23), (1, 384, 13), (2, 384, 15), (2, 208, 13), (1, 64, 13), (2, 64, 23)):
        rng = np.random.default_rng(7 * Z + R)
        Kb, ncols, ncore = kbits(BG, Z), O.NCOLS[(BG, R)], 26 if BG == 1 else 14
        for keep_cols in (ncols, ncore + 2.6):
            for kind in (1.0, 5.0, "rand"):
                llr = make_llr(rng, BG, Z, R, kind, random_info(rng, BG, Z, with_crc24b=True)).copy()
                llr[int(keep_cols * Z):] = 0
                for cap in (1, 8):
                    p = m.make_dec_params(BG, Z, R, cap, check_crc=True, E=Kb, crc_type=O.CRC24_B)
                    n, out = m.LDPCdecoder(p, llr, p_out=np.full(m.out_bytes(BG, Z, R), 0x33, np.uint8))
                    n_ref, out_ref = O.decode(BG, Z, R, llr, cap, 0, True, Kb, O.CRC24_B, out_init=0x33)
                    assert n == n_ref and np.array_equal(out, out_ref), (BG, Z, R, keep_cols, kind, cap, n, n_ref)
                    n_calls += 1
    after = m.server_stats()
    assert after["status"] == 0 and after["calls"] - before["calls"] == n_calls, (before, after, n_calls)
    BG, Z, R = 2, 208, 13
    llr = make_llr(np.random.default_rng(3), BG, Z, R, 3.0, random_info(np.random.default_rng(4), BG, Z, with_crc24b=True))
    seen = []

    def pred(ptr, n, t):
        seen.append(n)
        return O.check_crc(np.ctypeslib.as_array(ptr, shape=(n // 8 + 4,)), n, t)
    n_ref, out_ref = O.decode(BG, Z, R, llr, 8, 0, True, kbits(BG, Z), O.CRC24_B, out_init=0x33)
    p = m.make_dec_params(BG, Z, R, 8, check_crc=pred, E=kbits(BG, Z), crc_type=O.CRC24_B)
    n, out = m.LDPCdecoder(p, llr, p_out=np.full(out_ref.size, 0x33, np.uint8))
    assert n == n_ref and 3 <= n_ref < 9 and np.array_equal(out, out_ref), (n, n_ref)
    assert len(seen) == (0 if trust else n_ref - 2), (trust, seen)


def _ul_blocks():
    from test_gpu_tb_softbuf import _mk
    return [_mk(800, 2400, 2, 2, 1, 0),            # BG2 C=1
            _mk(5000, 14400, 2, 2, 1, 0),          # BG2 C=2
            _mk(3832, 9600, 1, 8, 1, 0),           # BG1 C=1, 256QAM
            _mk(9600, 33600, 1, 4, 1, 0),          # BG1 C=2
            _mk(20000, 26400, 1, 2, 1, 0),         # BG1 C=3, high rate: a first transmission on a cut graph
            _mk(9600, 33600, 1, 8, 1, 9000),       # limited-buffer rate matching
            _mk(5000, 40000, 2, 4, 1, 0)]          # repetition: E > N


@functools.lru_cache(maxsize=None)
def _ul_reference():
    """the 7 blocks, their payloads and soft buffers (dirty everywhere), the LLRs of two rounds (rv 0, then rv 2) and what the
    oracle's chain makes of them: per round the verdicts, the soft buffers and llrLen -- computed once, the probes copy"""
    from test_gpu_tb_softbuf import OracleChain, _noisy, _sigma, segs_of
    rng = np.random.default_rng(606)
    tbs = _ul_blocks()
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
    rows0 = rng.integers(-60, 60, (sum(segs_of(t) for t in tbs), O_HARQ_STRIDE)).astype(np.int16)
    ref = OracleChain(tbs, rows0)
    rounds = []
    for rnd, rv in ((0, 0), (1, 2)):
        for t in tbs:
            t["rv"], t["round"] = rv, rnd
            if rnd == 0:
                t["llrLen"] = 0
        llrs = [_noisy(rng, O.dlsch_encode(t, p), _sigma(t)) for t, p in zip(tbs, pays)]
        verdicts = [ref.decode(i, t, llrs[i], rnd) for i, t in enumerate(tbs)]
        rounds.append(dict(rnd=rnd, rv=rv, llrs=llrs, verdicts=verdicts, state=list(ref.state),
                           rows=np.concatenate([np.stack(d) for d in ref.d])))
    return tbs, pays, rows0, rounds


O_HARQ_STRIDE = 66 * 384


def test_probe_ul_chain(hip):
    """nrLDPC_hip_ulsch_decode on 7 small mixed transport blocks over two HARQ rounds at a noise level where some fail round 0:
    LLRs pageable, page-locked and in device memory, soft buffers in host and device memory; payloads, ACKs, pass counts,
    llrLen and every soft value of every row equal the oracle chain's."""
    from test_gpu_tb_softbuf import _check_verdicts, _decode, _harq_buffers, segs_of
    m = hip.ldpc
    assert m.HARQ_STRIDE == O_HARQ_STRIDE
    tbs0, pays, rows0, rounds = _ul_reference()
    assert sorted(segs_of(t) for t in tbs0) == [1, 1, 2, 2, 2, 2, 3] and {t["BG"] for t in tbs0} == {1, 2}
    acks0 = np.array([v[1] for v in rounds[0]["verdicts"]])
    acks1 = np.array([v[1] for v in rounds[1]["verdicts"]])
    assert 0 < acks0.sum() < len(tbs0) and (acks1 & ~acks0).any(), (acks0, acks1)      # some fail round 0, combining brings some back
    for mode in ("host", "pinned", "device", "harq_device"):
        tbs = [dict(t) for t in tbs0]
        harq = _harq_buffers(m, mode, rows0)
        for r in rounds:
            for t in tbs:
                t["rv"], t["round"] = r["rv"], r["rnd"]
                if r["rnd"] == 0:
                    t["llrLen"] = 0
            got = _decode(m, mode, tbs, r["llrs"], harq)
            for i, t in enumerate(tbs):
                _check_verdicts((mode, r["rnd"]), i, t, got, r["verdicts"][i], pays)
                assert t["llrLen"] == r["state"][i], (mode, r["rnd"], i)
            bad = np.argwhere(got[3] != r["rows"])
            assert bad.size == 0, (mode, r["rnd"], "first differing (row, position)", bad[:8].tolist())


def test_probe_dl_chain(hip):
    """nrLDPC_hip_dlsch_encode of blocks whose payload ends just before, at and just behind the 2 KiB and 8 KiB piece edges of the
    TB CRC kernel and spans several pieces; the plain encoder batch and LDPCencoder() on three codes."""
    from test_gpu_tb_chain import valid_tbs
    m = hip.ldpc
    rng = np.random.default_rng(2048)
    tbs = []
    # payload bytes; the TB CRC kernel walks payload + 3 CRC bytes: 2045 / 8189 / 16381 end exactly on a 2 KiB / 8 KiB piece edge,
    # 2047 puts the CRC across it, the others start a piece with a few bytes (only byte-aligned segmentations exist: valid_tbs)
    sizes = (2045, 2047, 2049, 4093, 4097, 6147, 8189, 8197, 16381, 16397)
    for nbytes in sizes:
        A = valid_tbs(8 * nbytes, 1)
        assert A == 8 * nbytes
        tbs.append(dict(A=A, G=2 * A, BG=1, Qm=2, Nl=1, rv=0, tbslbrm=0))
    tbs.append(dict(A=valid_tbs(8 * 300, 2), G=7200, BG=2, Qm=4, Nl=1, rv=0, tbslbrm=0))
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
    for f, t, p in zip(m.dlsch_encode_host(tbs, pays), tbs, pays):
        assert np.array_equal(f, O.dlsch_encode(t, p)), t
    for BG, Z in ((1, 384), (2, 64), (1, 36)):
        info = np.stack([random_info(rng, BG, Z) for _ in range(5)])
        ref = [O.encode(BG, Z, x) for x in info]
        assert np.array_equal(m.encode_batch_host(BG, Z, info), np.stack(ref)), (BG, Z)
        for o, r in zip(m.LDPCencoder(list(info), BG, Z), ref):
            assert np.array_equal(o, r), (BG, Z, "LDPCencoder")


def test_probe_evidence(hip):
    """in a child of test_switch_set: the library's own report shows the set in effect.  Every ("code_info", field, code) of the set
    differs from what the parent read in the default configuration and equals the table builder's value under this environment."""
    if EXPECT_ENV not in os.environ:
        for c in K.CODES:                                # the default configuration: library and builder agree
            fi = K.fast_info(*c)
            assert code_info_raw(hip.ldpc, *c) == dict({k: fi[k] for k in INFO_INDEX}, fast=1), c
        return
    exp = json.loads(os.environ[EXPECT_ENV])
    for kind, field, code in [e for e in exp["evidence"] if e[0] in ("code_info", "falls_back")]:
        got = code_info_raw(hip.ldpc, *code)[field]
        assert got != exp["defaults"]["%d,%d,%d" % tuple(code)][field], (exp["id"], field, code, got)
        if kind == "falls_back":
            assert got == 0 and _given_up(*code), (exp["id"], code, got)
        else:
            assert got == K.fast_info(*code)[field] and not _given_up(*code), (exp["id"], field, code, got)


# ---- the switch sets -----------------------------------------------------------------------------------------------------------------
_DIED = []          # the set whose child was killed by a signal, aborted or ran into its time limit: nothing more is started
_FAULT_WORDS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "Segmentation fault", "core dumped")
SET_SECONDS = {}    # measured per set (printed with -s / on failure)


def _child_limit(probes):
    """seconds: start-up of a fresh process (interpreter, torch, the build check, LDPCinit) plus four times what the set's probes
    took in this process; without a control run of a probe, a minute for it"""
    return 90.0 + 4.0 * sum(_CONTROL_SECONDS.get(PROBES[p], 60.0) for p in probes)


@pytest.mark.parametrize("sset", SWITCH_SETS, ids=[s["id"] for s in SWITCH_SETS])
def test_switch_set(hip, sset):
    """the set's probes in a fresh process under the set's environment: they pass, and the library reports the set in effect"""
    if _DIED:
        pytest.skip(f"the child of switch set {_DIED[0]} died; no further process is started")
    assert EXPECT_ENV not in os.environ, "this process is itself the child of a switch set: children select the probes only"
    # the parent is the control: it reads the defaults the child's evidence is compared with
    clash = [k for k in list(sset["env"]) + [K.PREFIX + k for k in K.KNOBS] if k in os.environ]
    assert not clash, f"{clash} set in this process' environment: the switch sets need the default configuration around them"
    defaults = {"%d,%d,%d" % c: code_info_raw(hip.ldpc, *c) for c in K.CODES}
    exp = dict(id=sset["id"], defaults=defaults, evidence=[e for e in sset["evidence"]])
    select = " or ".join([PROBES[p] for p in sset["probes"]] + ["test_probe_evidence"])
    limit = _child_limit(sset["probes"])
    cmd = [sys.executable, "-m", "pytest", str(HERE / "test_gpu_switches.py"), "-m", "gpu", "-q", "-x", "-s", "-p", "no:cacheprovider",
           "-k", select]
    t0 = time.perf_counter()
    try:
        r = subprocess.run(cmd, env=dict(os.environ, **sset["env"], **{EXPECT_ENV: json.dumps(exp)}), cwd=str(HERE.parent),
                           capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        _DIED.append(sset["id"])
        tail = "".join(x[-3000:] if isinstance(x, str) else x[-3000:].decode(errors="replace") for x in (e.stdout, e.stderr) if x)
        pytest.fail(f"switch set {sset['id']} {sset['env']}: no result within {limit:.0f} s\n{tail}")
    SET_SECONDS[sset["id"]] = time.perf_counter() - t0
    text = r.stdout[-4000:] + "\n--- stderr ---\n" + r.stderr[-3000:]
    what = f"switch set {sset['id']} {sset['env']} (probes {sset['probes']}, {SET_SECONDS[sset['id']]:.1f} s of {limit:.0f} s)"
    if r.returncode < 0 or r.returncode in (134, 139) or any(w in r.stdout or w in r.stderr for w in _FAULT_WORDS):
        _DIED.append(sset["id"])
        pytest.fail(f"{what}: the child died (exit status {r.returncode})\n{text}")
    assert r.returncode == 0, f"{what}: exit status {r.returncode}\n{text}"
    assert f"{len(sset['probes']) + 1} passed" in r.stdout, f"{what}: not every probe ran\n{text}"
    for e in sset["evidence"]:
        if e[0] == "stderr":
            assert e[1] in r.stderr, f"{what}: the library did not report {e[1]!r}\n{text}"
        if e[0] == "stderr_re":
            assert re.search(e[1], r.stderr), f"{what}: the library did not report {e[1]!r}\n{text}"
    print(f"{what}: ok")
