"""The decoder kernels on the CPU as they are written: tests/emul/dec_fast_emul.cpp includes ldpc_decoder.hip and
ldpc_decoder_fast.hip themselves against the host shim (tests/emul/hip_host/) and runs their own launchers with one real thread per
work-item -- the block bodies' queues, tickets, votes and barriers, the several-blocks-per-workgroup bodies, the pull prologue
and the launch dispatch, none of which the sequential walk of tests/emul/ldpc_emul.cpp has.  Everything is compared with the
oracle bit for bit: the pass count and every output byte, the criterion of the -m gpu tests.

Every case decodes blocks chosen with the oracle alone so that it cannot pass vacuously (choose_blocks): one that stops early,
one that fails after cap + 1 passes, a saturated one and a noiseless reference code word.  Which variant of the kernels a case
reaches is read from the descriptor the launch uses and asserted.  What this proves and what it cannot: DESIGN.md 4.16."""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import dec_emul_np as D
import oracle_lib as O
import switch_knobs as SK
from common import ALL_RATES, kbits, load_ref_code_words, make_llr, random_info

CAP = 8
FAST_SIZES = [Z for Z in O.LIFT_SIZES if Z % 4 == 0 and Z >= 8]
THROUGHPUT, LATENCY = 0, 1


@pytest.fixture(scope="module")
def dec(built):
    return D.lib()


@functools.lru_cache(maxsize=None)
def ref_code_word(BG, Z):
    kb = 22 if BG == 1 else 10
    for v in load_ref_code_words():
        if (v["BG"], v["Z"], v["Kb"]) == (BG, Z, kb):
            return v["coded"]
    raise AssertionError(("no reference code word", BG, Z))


def oracle(BG, Z, R, llr, mode, crc):
    return O.decode(BG, Z, R, llr, CAP, mode, crc, kbits(BG, Z) if crc else 0, O.CRC24_B, out_init=D.OUT_INIT)


@functools.lru_cache(maxsize=None)
def choose_blocks(BG, Z, R, crc):
    """Four decoder inputs picked with the oracle alone: {early stop with 3 <= passes <= cap, all cap + 1 passes and failed,
    saturated, noiseless reference code word}; asserted here, so that no case can pass on blocks that all behave alike."""
    rng = np.random.default_rng(1000 * BG + 7 * Z + R + (50000 if crc else 0))
    n = O.NCOLS[(BG, R)] * Z
    early = fail = None
    for snr in (1.5, 1.0, 0.5, 0.0, -0.5, -1.0, -1.5, -2.0, -3.0, 2.5, 3.5, -4.0, 5.0) * 6:
        llr = make_llr(rng, BG, Z, R, snr, random_info(rng, BG, Z, with_crc24b=True))[:n]
        it = oracle(BG, Z, R, llr, 0, crc)[0]
        if early is None and 3 <= it <= CAP:
            early = llr
        if fail is None and it == CAP + 1:
            fail = llr
        if early is not None and fail is not None:
            break
    assert early is not None and fail is not None, (BG, Z, R, crc)
    sat = rng.choice(np.array([-128, -127, 127, 127, -128, 0, 1, -1], dtype=np.int8), n)
    assert (sat == 127).any() and (sat == -127).any() and (sat == -128).any()
    cw = ref_code_word(BG, Z)[:n - 2 * Z]
    clean = np.concatenate([np.zeros(2 * Z, np.int8), np.where(cw == 0, 20, -20).astype(np.int8)])
    llrs = np.ascontiguousarray(np.stack([early, fail, sat, clean]), np.int8)
    llrs.setflags(write=False)
    return llrs


@functools.lru_cache(maxsize=None)
def expected(BG, Z, R, mode, crc):
    llrs = choose_blocks(BG, Z, R, crc)
    ref = [oracle(BG, Z, R, l, mode, crc) for l in llrs]
    its = [r[0] for r in ref]
    assert 3 <= its[0] <= CAP and its[1] == CAP + 1, its
    return llrs, np.array(its, np.int32), np.stack([r[1] for r in ref])


def check(kernel, BG, Z, R, mode=0, crc=False, shape=THROUGHPUT, walk=None, **kw):
    """the emulated launch == the oracle (and == the sequential walk of ldpc_emul.cpp for the one-block fast kernel)"""
    llrs, its, outs = expected(BG, Z, R, mode, crc)
    p = D.params(kernel=kernel, BG=BG, Z=Z, R=R, shape=shape, n_blocks=len(llrs), max_iter=CAP, out_mode=mode, use_crc=crc,
                 E=kbits(BG, Z) if crc else 0, crc_type=O.CRC24_B, **kw)
    rc, n_iter, out = D.decode_p(p, llrs, outs.shape[1])
    key = (kernel, BG, Z, R, mode, crc, shape, kw)
    assert rc == 0, key
    assert np.array_equal(n_iter, its), key + (n_iter.tolist(), its.tolist())
    assert np.array_equal(out, outs), key
    if walk is not None:
        L = SK.emul_lib()
        L.ldpc_emul_set_fast_shape(shape)
        for k, llr in enumerate(llrs):
            o = np.full(outs.shape[1], D.OUT_INIT, np.uint8)
            n = L.ldpc_emul_decode_fast(BG, Z, R, CAP, mode, int(crc), kbits(BG, Z) if crc else 0, O.CRC24_B, llr.ctypes.data, o.ctypes.data)
            assert n == n_iter[k] and np.array_equal(o, out[k]), key + ("walk", k)
        L.ldpc_emul_set_fast_shape(THROUGHPUT)
    return n_iter, out


def smallest(pred, kernel=D.KERNEL_FAST, shape=THROUGHPUT, sizes=FAST_SIZES, bgs=(1, 2)):
    """the smallest (Z, then BG, then rate mode as listed) whose descriptor satisfies pred"""
    for Z in sizes:
        for BG in bgs:
            for R in ALL_RATES[BG]:
                i = D.info(kernel, BG, Z, R, shape)
                if i and (kernel == D.KERNEL_GENERIC or i["F_OK"]) and pred(i):
                    return BG, Z, R, i
    raise AssertionError("no code reaches the variant")


@pytest.mark.parametrize("shape", [THROUGHPUT, LATENCY])
@pytest.mark.parametrize("Z", [8, 44])
@pytest.mark.parametrize("BG", [1, 2])
def test_single_task_codes(dec, BG, Z, shape):
    """single check-node tasks only; Zc = 8 and Zc = 44, whose rows of 11 items leave the last wave of a task partial; both
    workgroup shapes; every rate mode once per case: one of them through the CRC instantiation (packed bits: the reference checks
    the CRC on the output row; which rate mode moves with the case, so that each meets it), the others through the syndrome
    instantiation with the other two output modes"""
    crc_at = (BG + Z // 44 + shape) % 3
    for k, R in enumerate(ALL_RATES[BG]):
        i = D.info(D.KERNEL_FAST, BG, Z, R, shape)
        assert i["F_OK"] and i["DOUBLE_TASKS"] == 0 and i["MB"] == 1 and i["SUB"] == 1
        assert i["ZQ"] == Z // 4 and (Z != 44 or i["ZQ"] % 64 == 11)
        if k == crc_at:
            check(D.KERNEL_FAST, BG, Z, R, crc=True, shape=shape, walk=True)
        else:
            check(D.KERNEL_FAST, BG, Z, R, mode=(k - crc_at) % 3, crc=False, shape=shape, walk=True)


@pytest.mark.parametrize("BG,Z,R", [(2, 256, 15), (1, 256, 13), (2, 288, 15)])
def test_double_tasks(dec, BG, Z, R):
    """extension rows in double tasks (items lane and lane + 64 through ldpc_fast_cn2_dispatch), among them one with fewer than
    128 items, whose upper threads take their first item twice.  Zc = 256 is the smallest lifting size that has any; its rows
    are 64 items long, so the two items of a thread always sit at the same place j of two neighbouring rows -- Zc = 288 (rows of
    72) is the smallest where they do not, and where mixing up the two items' j is seen"""
    i = D.info(D.KERNEL_FAST, BG, Z, R)
    assert i["F_OK"] and i["DOUBLE_TASKS"] >= 1 and i["SHORT_DOUBLE_TASKS"] >= 1 and i["ZQ"] == Z // 4, i
    if Z == 256:
        for z in FAST_SIZES:                                # ... and no smaller lifting size has any
            if z < 256:
                assert D.info(D.KERNEL_FAST, BG, z, R)["DOUBLE_TASKS"] == 0, z
    check(D.KERNEL_FAST, BG, Z, R, crc=False, walk=True)
    if (BG, Z) == (2, 256):
        check(D.KERNEL_FAST, BG, Z, R, crc=True, zc=0, jobs=1)    # the general jobs kernel (the launcher's zc = 0)


def test_pair19_rows_on_the_host(dec):
    """f_pair19: two lanes share a degree-19 item on the device (ldpc_fast_cn19_pair, device code only); the host build gives the
    item to the even lane and nothing to the odd one (ldpc_dec_fast_block.h)"""
    BG, Z, R, i = smallest(lambda i: i["PAIR19"], bgs=(1,))
    assert i["PAIR19"] == 1
    for shape in (THROUGHPUT, LATENCY):
        if D.info(D.KERNEL_FAST, BG, Z, R, shape)["PAIR19"]:
            check(D.KERNEL_FAST, BG, Z, R, crc=shape == LATENCY, shape=shape, walk=True)


def test_extension_llrs_in_memory_and_in_lds(dec):
    """f_ext_global = 0 (the extension columns' LLRs staged in LDS) and = 1 (read from the block's row in memory every pass): the
    smallest code of each kind in the throughput shape; where the builder's default gives one kind only, the other through
    NRLDPC_HIP_EXT_GLOBAL"""
    seen = set()
    for want in (0, 1):
        env = {}
        try:
            BG, Z, R, i = smallest(lambda i: i["EXT_GLOBAL"] == want, sizes=[Z for Z in FAST_SIZES if Z <= 64])
        except AssertionError:
            env = {"EXT_GLOBAL": str(want)}
            with SK.knob_env(env):
                BG, Z, R, i = smallest(lambda i: i["EXT_GLOBAL"] == want)
        with SK.knob_env(env):
            assert D.info(D.KERNEL_FAST, BG, Z, R)["EXT_GLOBAL"] == want
            check(D.KERNEL_FAST, BG, Z, R, walk=True)
            if want:
                check(D.KERNEL_FAST, BG, Z, R, crc=True, walk=True)
        seen.add(want)
    assert seen == {0, 1}


def test_grouped_bit_node_tickets(dec):
    """bit-node tickets that hold several short tasks (f_bn_ticket[.][1] > 1: ldpc_fast_bn_multi, fillers for the tasks a ticket
    does not have) and descriptors with f_bn_group > 1: the smallest code with each"""
    BG, Z, R, i = smallest(lambda i: i["BN_TICKET_MAX"] > 1)
    assert i["BN_TICKET_MAX"] > 1
    check(D.KERNEL_FAST, BG, Z, R, walk=True)
    BG, Z, R, i = smallest(lambda i: i["BN_GROUP"] > 1)
    assert i["BN_GROUP"] > 1
    check(D.KERNEL_FAST, BG, Z, R, crc=True, walk=True)


def test_lifting_size_instantiation_against_the_general_kernel(dec, tmp_path):
    """Zc = 208, the smallest of LDPC_FAST_ZC_LIST: ldpc_launch_dec_fast takes ldpc_launch_zc's instantiation (compile-time row
    strides) here and the general kernel in a child process with NRLDPC_HIP_ZC=0 (the switch is read once per process); the
    jobs launcher takes either by its zc argument.  All of them equal the oracle, hence each other."""
    BG, Z, R = 1, 208, 89
    assert dec.dec_emul_takes_zc_kernel(BG, Z, R, THROUGHPUT) == 1
    n_iter, out = check(D.KERNEL_FAST, BG, Z, R, walk=True)
    for zc in (Z, 0):
        check(D.KERNEL_FAST, BG, Z, R, crc=True, jobs=1, zc=zc)
    check(D.KERNEL_FAST, BG, Z, R, jobs=1, zc=Z)
    llrs, its, outs = expected(BG, Z, R, 0, False)
    p = D.params(kernel=D.KERNEL_FAST, BG=BG, Z=Z, R=R, n_blocks=len(llrs), max_iter=CAP)
    np.savez(tmp_path / "in.npz", p=p, llr=llrs, out_bytes=outs.shape[1])
    env = dict(os.environ, NRLDPC_HIP_ZC="0")
    subprocess.run([sys.executable, str(Path(D.__file__)), str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], check=True, env=env, timeout=120)
    z = np.load(tmp_path / "out.npz")
    assert int(z["takes_zc"]) == 0 and int(z["rc"]) == 0
    assert np.array_equal(z["n_iter"], n_iter) and np.array_equal(z["out"], out)


def test_jobs_of_mixed_codes_and_the_abort_flag(dec):
    """ldpc_dec_fast_kernel<true, .> on four jobs of different (BG, Zc <= 64) in one launch, each with a workgroup as large as the
    largest code's: pass counts scattered through iter_idx; two jobs share a transport-block flag and the first of them fails,
    so its sibling -- the runner executes workgroups in order -- gives up at its second pass: numMaxIter + 2, nothing written.
    oracle_lib decodes one block at a time and has no transport-block abort, so that rule (nrLDPC_decoder.c:556-559, as
    ldpc_dec_fast_block.h states it) is restated here by hand: CAP + 2 and an untouched row for the sibling; every other job,
    and every job of the same launch without the flag, equals the oracle"""
    J = D.names("J")
    codes = [(1, 16, 13), (2, 64, 15), (1, 44, 23), (2, 8, 13)]
    picks = [1, 0, 0, 2]                                     # job 0: the failing block; its sibling job 1 would stop early
    for crc in (True, False):
        for use_abort in (True, False):
            llr_rows, refs, llr_off, out_off, spec = [], [], [], [], np.zeros((4, J["COUNT"]), np.int32)
            lo = oo = 0
            for k, ((BG, Z, R), pick) in enumerate(zip(codes, picks)):
                llrs, its, outs = expected(BG, Z, R, 0, crc)
                llr_rows.append(llrs[pick]); refs.append((its[pick], outs[pick]))
                llr_off.append(lo); out_off.append(oo)
                lo += (llrs.shape[1] + 15) // 16 * 16; oo += (outs.shape[1] + 15) // 16 * 16
                spec[k, [J["BG"], J["Z"], J["R"], J["MAX_ITER"], J["E"], J["CRC_TYPE"], J["ITER_IDX"], J["ABORT_IDX"]]] = \
                    [BG, Z, R, CAP, kbits(BG, Z) if crc else 0, O.CRC24_B, 3 - k, (0 if k < 2 else -1) if use_abort else -1]
            assert refs[0][0] == CAP + 1 and 3 <= refs[1][0] <= CAP
            llr = np.zeros(lo, np.int8)
            for o, row in zip(llr_off, llr_rows):
                llr[o:o + row.size] = row
            out = np.full(oo, D.OUT_INIT, np.uint8)
            n_iter = np.full(4, -7, np.int32)
            flags = np.zeros(2, np.int32)
            lo_a, oo_a = np.array(llr_off, np.uint64), np.array(out_off, np.uint64)
            rc = dec.dec_emul_decode_jobs(1, 4, spec.ctypes.data, lo_a.ctypes.data, oo_a.ctypes.data,
                                          THROUGHPUT, 0, int(crc), 0, llr.ctypes.data, out.ctypes.data, n_iter.ctypes.data,
                                          flags.ctypes.data if use_abort else None)
            assert rc == 0
            for k, (it, o) in enumerate(refs):
                got = out[out_off[k]:out_off[k] + o.size]
                if use_abort and k == 1:
                    assert n_iter[3 - k] == CAP + 2 and (got == D.OUT_INIT).all(), (crc, n_iter.tolist())
                else:
                    assert n_iter[3 - k] == it and np.array_equal(got, o), (crc, use_abort, k, n_iter.tolist())
            assert flags.tolist() == ([1, 0] if use_abort else [0, 0])


@pytest.mark.parametrize("crc", [False, True])
def test_pull_kernel(dec, crc):
    """ldpc_dec_fast_pull_kernel at Zc = 16: rows the workgroup copies into the launch's device rows in 16-byte units (source and
    destination 16-byte aligned) or in dwords (the source 4 bytes off), with and without the first round's stagger; the device
    rows end up equal to the source and the decode equals the oracle.  The four combinations of alignment and stagger are split over
    the two parametrisations: the syndrome instantiation runs (aligned, no stagger) and (misaligned, staggered), the CRC one
    (aligned, staggered) and (misaligned, no stagger)"""
    BG, Z, R = 2, 16, 13
    llrs, its, outs = expected(BG, Z, R, 0, crc)
    n, nl = llrs.shape
    stride = (nl + 15) // 16 * 16
    for off in (0, 4):
        for stagger in ((0, 3) if off == 0 else (3, 0))[crc:crc + 1]:
            raw = np.zeros(n * stride + 32, np.int8)
            base = (-raw.ctypes.data) % 16 + off
            src = raw[base:base + n * stride].reshape(n, stride)
            src[:, :nl] = llrs
            dst_raw = np.full(n * stride + 16, 0x11, np.int8)
            dbase = (-dst_raw.ctypes.data) % 16
            dst = dst_raw[dbase:dbase + n * stride]
            assert src.ctypes.data % 16 == off and dst.ctypes.data % 16 == 0
            p = D.params(kernel=D.KERNEL_PULL, BG=BG, Z=Z, R=R, n_blocks=n, max_iter=CAP, use_crc=crc, E=kbits(BG, Z) if crc else 0,
                         crc_type=O.CRC24_B, pull_stagger=stagger, pull_first_round=n)
            out = np.full((n, outs.shape[1]), D.OUT_INIT, np.uint8)
            n_iter = np.full(n, -7, np.int32)
            rc = dec.dec_emul_decode(p.ctypes.data, dst.ctypes.data, stride, out.ctypes.data, outs.shape[1], n_iter.ctypes.data,
                                     src.ctypes.data, stride, None)
            assert rc == 0
            assert np.array_equal(dst.reshape(n, stride)[:, :nl], llrs) and (dst.reshape(n, stride)[:, nl:] == 0x11).all(), (off, stagger)
            assert np.array_equal(n_iter, its) and np.array_equal(out, outs), (off, stagger, n_iter.tolist())


def multi_case(BG, Z, R, crc, jobs, mode=0, mb=0, counts=(-1, 0, 1)):
    """several blocks per workgroup (mb: f_mb asked of the builder, 0: the library's choice for the lifting size): per_wg - 1,
    per_wg and per_wg + 1 blocks (a ragged last workgroup, a workgroup of one block), the four chosen blocks repeated in an
    order that mixes pass counts inside every workgroup"""
    i = D.info(D.KERNEL_MULTI, BG, Z, R, THROUGHPUT, mb)
    assert i["F_OK"] and i["MB"] >= 2 and (mb == 0 or i["MB"] == mb)
    per_wg = i["MB"] * i["SUB"]
    llrs, its, outs = expected(BG, Z, R, mode, crc)
    for n in (per_wg + d for d in counts):
        order = [(3 * k + k // 4) % 4 for k in range(n)]
        assert len(set(order[:per_wg - 1])) >= min(4, per_wg - 1)
        p = D.params(kernel=D.KERNEL_MULTI, BG=BG, Z=Z, R=R, n_blocks=n, max_iter=CAP, out_mode=mode, use_crc=crc,
                     E=kbits(BG, Z) if crc else 0, crc_type=O.CRC24_B, jobs=jobs, mb=mb)
        rc, n_iter, out = D.decode_p(p, np.ascontiguousarray(llrs[order]), outs.shape[1])
        assert rc == 0
        assert np.array_equal(n_iter, its[order]), (BG, Z, R, crc, jobs, n, n_iter.tolist())
        assert np.array_equal(out, outs[order]), (BG, Z, R, crc, jobs, n)
    return i


@pytest.mark.parametrize("jobs", [0, 1])
def test_several_blocks_per_workgroup(dec, jobs):
    """ldpc_dec_fast_multi_kernel<1> / _multi_jobs_kernel<1> (jobs): the smallest lifting size whose descriptor puts f_mb >= 2
    blocks side by side in a workgroup.  The three block counts with four blocks per workgroup (f_mb = 4: every kind of block in
    each), and one ragged launch with as many as the library takes for the lifting size"""
    BG, Z, R, i = smallest(lambda i: i["MB"] >= 2 and i["SUB"] == 1, kernel=D.KERNEL_MULTI, bgs=(2,))
    assert Z == 8 and i["MB"] >= 2 and i["SUB"] == 1
    multi_case(BG, Z, R, crc=bool(jobs), jobs=jobs, mb=4)
    multi_case(BG, Z, R, crc=not jobs, jobs=jobs, mb=4, counts=(1,))
    multi_case(BG, Z, R, crc=False, jobs=jobs, mode=1 + jobs, counts=(1,))


@pytest.mark.parametrize("jobs", [0, 1])
def test_four_interleaved_blocks_per_group(dec, jobs):
    """ldpc_dec_fast_multi_kernel<4> / _multi_jobs_kernel<4>: lifting sizes the one-block fast kernel does not take, four blocks
    byte-interleaved into one of a virtual code (f_sub = 4); a block's row is written at the moment it stops.  The three block
    counts with two groups per workgroup (f_mb = 2), one ragged launch with the library's sixteen groups, and the CRC stop at
    Zc = 4, the smallest such lifting size whose K is a whole number of bytes and >= 48 bits"""
    BG, Z, R, i = smallest(lambda i: i["SUB"] == 4, kernel=D.KERNEL_MULTI, sizes=O.LIFT_SIZES, bgs=(2,))
    assert Z == 2 and i["SUB"] == 4
    multi_case(BG, Z, R, crc=False, jobs=jobs, mb=2)
    multi_case(BG, Z, R, crc=False, jobs=jobs, mode=1 + jobs, counts=(1,))
    assert D.info(D.KERNEL_MULTI, 1, 4, 23, THROUGHPUT, 2)["SUB"] == 4
    multi_case(1, 4, 23, crc=True, jobs=jobs, mb=2, counts=(-1, 1))


def test_eager_parity_sweep(dec):
    """the homogeneous launches evaluate a pass' parity check in a sweep of its own when the block is close (eager_check());
    the jobs launches fold it into the next pass.  Latency shape, the diagnostic instantiation's stamps say in which passes the
    sweep ran: it did, for the block that stops early, and the pass counts equal the jobs launch's and the oracle's"""
    BG, Z, R = 1, 44, 23
    llrs, its, outs = expected(BG, Z, R, 0, False)
    trace = np.zeros((len(llrs), 32), np.uint64)
    p = D.params(kernel=D.KERNEL_FAST, BG=BG, Z=Z, R=R, shape=LATENCY, n_blocks=len(llrs), max_iter=CAP)
    rc, n_iter, out = D.decode_p(p, llrs, outs.shape[1], trace=trace)
    assert rc == 0 and np.array_equal(n_iter, its) and np.array_equal(out, outs)
    stamps = trace.view(np.uint32).reshape(len(llrs), 64)[:, 10:]          # ldpc_batch_io::stamps(): behind five 64-bit words
    swept = stamps[:, 20]
    assert swept[0] & (1 << int(its[0])), (swept.tolist(), its.tolist())   # the stop of block 0 was found by the sweep of its last pass
    assert (trace[:, 4] == its.astype(np.uint64)).all()
    check(D.KERNEL_FAST, BG, Z, R, shape=LATENCY, jobs=1)


@pytest.mark.parametrize("Z", [2, 3, 6])
def test_generic_kernel(dec, Z):
    """ldpc_decoder.hip / ldpc_dec_generic_block.h at lifting sizes the fast kernel does not take (Z & 3, or Z < 8): both base
    graphs at each, a rate mode each that moves with the lifting size (the three cases run every rate mode of both), batch and
    jobs launcher, the three output modes.  (No CRC stop here: K is no whole number of bytes >= 48 bits at these sizes; the
    fast kernels' cases run it.)"""
    zi = (2, 3, 6).index(Z)
    for BG in (1, 2):
        R = ALL_RATES[BG][(zi + BG) % 3]
        i = D.info(D.KERNEL_GENERIC, BG, Z, R)
        assert i["F_OK"] == 0 and (Z & 3 or Z < 8)
        assert not (kbits(BG, Z) % 8 == 0 and kbits(BG, Z) >= 48)
        check(D.KERNEL_GENERIC, BG, Z, R, mode=(zi + BG) % 3, jobs=(zi + BG) & 1)


# ---- the fused UL segment kernel (tb_rx_fused.hip through tests/emul/rx_fused_emul.cpp) ------------------------------------------
# Everything is compared with the oracle's UL-SCH chain (O.ulsch_decode), as tests/test_gpu_tb_chain.py compares: payload bytes, ACK,
# iter_max, per-segment pass counts and the int16 soft buffers over the whole row.  The runner executes workgroups one after the
# other: the segment that finishes a transport block last finds every slot written, so the spin loop in the epilogue
# (tb_rx_fused.hip, "while (... >> 48 != gen)") is never seen spinning here, and an abort flag raised by a segment is always seen
# by the segments behind it.

def fused_tb(bits, BG, C_, rate, Qm=2, Z=None):
    """the smallest byte-aligned transport block of at least `bits` bits with C_ segments (and lifting size Z), at code rate `rate`"""
    A = (bits + 7) // 8 * 8
    while True:
        B = O.len_with_crc(1, A)
        s = O.segmentation(None, B, BG)
        L = 24 if s["C"] > 1 else 0
        if (s["K"] - s["F"] - L) % 8 == 0 and s["F"] % 8 == 0 and (B + L * s["C"]) % s["C"] == 0 and s["C"] == C_ and Z in (None, s["Z"]):
            break
        A += 8
        assert A < bits + 4000, (bits, BG, C_, Z)
    G = int(A / rate) // (Qm * C_) * Qm * C_
    return dict(A=A, G=G, BG=BG, Qm=Qm, Nl=1, rv=0, round=0, tbslbrm=0, llrLen=0, C=C_, Z=s["Z"])


def channel(rng, t, payload, sigma):
    f = O.dlsch_encode(t, payload)
    return np.clip(np.round((1 - 2 * f.astype(np.float64)) * 8 + sigma * rng.standard_normal(f.size)), -200, 200).astype(np.int16)


class FusedState:
    """transport blocks with the emulation's and the oracle's soft buffers side by side, from round to round"""

    def __init__(self, tbs, seed):
        self.tbs, self.rng = tbs, np.random.default_rng(seed)
        self.ref_tbs = [dict(t) for t in tbs]
        self.pays = [self.rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
        n = sum(t["C"] for t in tbs)
        self.harq = np.zeros((n, D.HARQ_STRIDE), np.int16)
        self.harq_ref = [[np.zeros(D.HARQ_STRIDE, np.int16) for _ in range(t["C"])] for t in tbs]
        self.gen = np.zeros(len(tbs), np.uint32)
        self.llr_len_ref = [0] * len(tbs)

    def llrs(self, rv, rnd, sigma, spoil=()):
        out = []
        for i, (t, p) in enumerate(zip(self.tbs, self.pays)):
            t["rv"], t["round"] = rv, rnd
            f = channel(self.rng, t, p, sigma)
            for (ti, r) in spoil:                                  # segment r of block ti: noise alone
                if ti == i:
                    E0 = sum(O.get_E(t["G"], t["C"], t["Qm"], t["Nl"], q) for q in range(r))
                    E = O.get_E(t["G"], t["C"], t["Qm"], t["Nl"], r)
                    f[E0:E0 + E] = np.round(6 * self.rng.standard_normal(E)).astype(np.int16)
            out.append(f)
        return out

    def oracle(self, llrs, rnd, cap=CAP):
        res = []
        for i, t in enumerate(self.tbs):
            p, ack, its, self.llr_len_ref[i] = O.ulsch_decode(t, llrs[i], self.harq_ref[i], cap, rnd, self.llr_len_ref[i])
            res.append((p, ack, its))
        return res

    def check(self, got, ref, key, cap=CAP):
        assert got["rc"] == 0, (key, got["rc"])
        row = 0
        for i, (t, (p_ref, ack_ref, its)) in enumerate(zip(self.tbs, ref)):
            seg_it = got["seg"]["ITER"][row:row + t["C"]].tolist()
            assert bool(got["ack"][i]) == ack_ref, (key, i, its, seg_it)
            assert got["iter_max"][i] == min(max(its), cap + 1), (key, i, its, int(got["iter_max"][i]))
            assert t["llrLen"] == self.llr_len_ref[i], (key, i)
            if max(its) <= cap:
                assert seg_it == its, (key, i, its, seg_it)
            else:                                                  # siblings behind a failed segment give up: cap + 2
                assert all(a == b or a == cap + 2 for a, b in zip(seg_it, its)) and cap + 1 in seg_it, (key, i, its, seg_it)
            if ack_ref:
                assert np.array_equal(got["payload"][i], p_ref) and np.array_equal(p_ref, self.pays[i]), (key, i)
            else:
                assert not got["payload"][i].any(), (key, i)       # a failed block delivers zeros
            for r in range(t["C"]):
                assert np.array_equal(self.harq[row + r], self.harq_ref[i][r]), (key, i, r)
            row += t["C"]


@functools.lru_cache(maxsize=None)
def fused_blocks():
    """1, 2 and 3 segments: a small single BG2 segment, and the smallest multi-segment blocks -- BG2: two segments of Zc = 208, the
    smallest lifting size with instantiations of its own, and three of Zc = 288 (three BG2 segments have at least that)"""
    return (fused_tb(400, 2, 1, 0.80), fused_tb(3900, 2, 2, 0.80, Z=208), fused_tb(7640, 2, 3, 0.80, Z=288))


@pytest.mark.parametrize("lrow", [1, 0])
def test_fused_first_transmission_on_the_cut_graph(dec, lrow):
    """first transmissions at rate 0.8: segments decoded on the rate mode's graph cut behind the last column they reach, blocks
    of 1, 2 and 3 segments in one launch (mixed lifting sizes: the general kernel), the decoder input in LDS (LROW) and in memory;
    then the Zc = 208 block alone through the lifting size's own instantiation; at a noise level where every block decodes
    in 3 passes or more and at one where some fail"""
    seen = set()
    for sigma, seed in ((2.2, 11), (4.2, 12), (5.2, 13)):
        for pick, zc in (((0, 1, 2), 0), ((1,), 1)):
            st = FusedState([dict(fused_blocks()[k]) for k in pick], seed)
            llrs = st.llrs(0, 0, sigma)
            ref = st.oracle(llrs, 0)
            got = D.fused_run(st.tbs, llrs, st.harq, st.gen, lrow=lrow, zc=zc)
            assert got["info"]["N_CUT"] >= 1 and bool(got["info"]["LROW_OFF"]) == bool(lrow), got["info"]
            assert got["info"]["ZC"] == (208 if zc else 0) and got["info"]["MUTE"] == 0, got["info"]
            st.check(got, ref, (lrow, sigma, pick))
            assert (st.gen == 1).all()
            seen |= {(bool(a), max(its)) for _, a, its in ref}
    assert any(a and n >= 3 for a, n in seen) and any(not a for a, n in seen), seen


def test_fused_rv_0_2_3_with_combining_and_mute_items(dec):
    """rv 0 -> 2 -> 3 on the same soft buffers at a noise level where the first round fails: every round equals the oracle's
    chain (payload, ACK, pass counts, soft buffers, llrLen).  The retransmissions run the MUTE instantiation: the rv 2 round's
    decoder input -- asserted from the rows themselves -- has extension-row items whose four LLRs are all zero (holes no
    transmission has reached) and items that are not; the same rounds with the mute check off, and with the decoder input in
    LDS, give the same results"""
    runs = {}
    for name, opts in (("mute", dict(mute=1, lrow=0)), ("plain", dict(mute=0, lrow=0)), ("lrow", dict(mute=1, lrow=1, zc=1))):
        st = FusedState([dict(fused_blocks()[k]) for k in (1, 2)], 21)
        out = []
        for rnd, rv, sigma in ((0, 0, 5.5), (1, 2, 5.0), (2, 3, 4.0)):
            llrs = st.llrs(rv, rnd, sigma)
            ref = st.oracle(llrs, rnd)
            got = D.fused_run(st.tbs, llrs, st.harq, st.gen, want_rows=not opts["lrow"], **opts)
            st.check(got, ref, (name, rnd))
            assert got["info"]["MUTE"] == (1 if rnd and opts["mute"] else 0), (name, rnd, got["info"])
            if rnd == 1 and name == "mute":
                mute = live = 0
                for k in range(got["info"]["N_SEG"]):
                    Z, nc, nl = (int(got["seg"][f][k]) for f in ("Z", "NCORE", "NUM_LLR"))
                    ext = got["rows"][k, nc * Z:nl].reshape(-1, 4)          # Z % 4 == 0: an item is four lanes of one column
                    mute += int((ext == 0).all(axis=1).sum())
                    live += int((ext != 0).any(axis=1).sum())
                    assert (got["rows"][k, nl:] == 0x11).all()
                assert mute >= 1 and live >= 1, (mute, live)
            out.append((got["ack"].tolist(), got["iter_max"].tolist(), got["seg"]["ITER"].tolist(), [p.tobytes() for p in got["payload"]]))
        assert not all(out[0][0]) and all(out[2][0]), out                  # the first round fails, combining decodes
        runs[name] = (out, st.harq.copy())
    assert runs["mute"][0] == runs["plain"][0] == runs["lrow"][0]
    assert np.array_equal(runs["mute"][1], runs["plain"][1]) and np.array_equal(runs["mute"][1], runs["lrow"][1])


def test_fused_failed_segment_and_interleaved_blocks(dec):
    """two transport blocks (3 and 2 segments) whose segments alternate in workgroup order, so that each block's verdict is
    delivered by whichever of its segments finishes last ("last to finish collects"); one segment of the first block is noise
    alone: ACK 0, the payload zeroed although its siblings decoded, iter_max capped at cap + 1; the other block is untouched by
    it.  A second call on the same blocks (an rv 2 round on the same soft buffers, generation 2) equals the oracle again.
    The runner executes workgroups one after the other, which is enough for the epilogue -- the last arriver finds every slot
    written -- and means that the spin loop that waits for a slot's generation (tb_rx_fused.hip, tb_finish: "while (... >> 48 !=
    (gen & 0xffff))") is never seen spinning here"""
    st = FusedState([dict(fused_blocks()[2]), dict(fused_blocks()[1])], 31)
    llrs = st.llrs(0, 0, 2.0, spoil=((0, 1),))
    ref = st.oracle(llrs, 0)
    assert not ref[0][1] and ref[0][2][1] == CAP + 1 and max(ref[0][2][0], ref[0][2][2]) <= CAP and ref[1][1]
    got = D.fused_run(st.tbs, llrs, st.harq, st.gen, interleave=1, lrow=1)
    st.check(got, ref, "failed")
    assert got["ack"].tolist() == [0, 1] and got["iter_max"][0] == CAP + 1 and not got["payload"][0].any()
    assert st.gen.tolist() == [1, 1]
    llrs = st.llrs(2, 1, 2.0)
    ref = st.oracle(llrs, 1)
    got = D.fused_run(st.tbs, llrs, st.harq, st.gen, interleave=1, lrow=1)
    st.check(got, ref, "again")
    assert got["ack"][1] == 1 and st.gen.tolist() == [2, 2]


def test_fused_scrambled_codeword(dec):
    """the SCR and SYM instantiations: the blocks' LLRs are a scrambled codeword each (c_init), unscrambled in the prologue, or
    come as the block's symbol record, demapped and unscrambled there; equal to the oracle's chain on the unscrambled LLRs, with
    the decoder input in LDS and in memory"""
    from test_scrambling_host import serial_gold
    st = FusedState([dict(fused_blocks()[0], c_init=0x1234567), dict(fused_blocks()[1], c_init=0x7654321 & 0x7fffffff)], 41)
    llrs = st.llrs(0, 0, 2.4)
    ref = st.oracle(llrs, 0)
    scrambled = []
    for t, f in zip(st.tbs, llrs):
        c = serial_gold(t["c_init"], f.size).astype(bool)
        g = f.copy()
        g[c] = -g[c]
        scrambled.append(g)
    # SYM: each block's symbol record instead of its LLRs.  QPSK: one plane of (re, im) words, and the demapper's LLR is y >> 3
    # (tests/qam_np.py demap_np, the definition), so the record y = 8 f demaps to the scrambled LLRs f exactly
    from qam_np import demap_np
    records = [(8 * g.astype(np.int32)).astype(np.int16) for g in scrambled]
    for g, rec in zip(scrambled, records):
        assert np.array_equal(demap_np(rec.reshape(-1, 2), [], 2), g)
    for lrow, sym in ((1, 0), (0, 0), (1, 1), (0, 1)):
        st.harq[:] = 0
        for t in st.tbs:
            t["llrLen"] = 0
        got = D.fused_run(st.tbs, records if sym else scrambled, st.harq, st.gen, scr=1, sym=sym, lrow=lrow)
        st.check(got, ref, ("scr", lrow, sym))
