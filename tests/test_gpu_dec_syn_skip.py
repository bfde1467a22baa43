"""-m gpu: the fast decoder's parity-check skip (ldpc_dec_fast_block.h, "the queue word of a pass") against the oracle.  Once the
running count of a pass' unsatisfied lanes has passed LDPC_EAGER_MAX_BAD_LANES, the check-node tasks drawn behind that point run
without the parity; which tasks those are depends on the order the waves happen to run in, the pass counts and output bytes must
not.  Batches that mix blocks which stop at different passes, fail, or are noiseless, launched repeatedly; and the diagnostic
instantiation's trace rows, which say in which passes tasks ran without the parity."""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as O
from common import kbits, make_llr, random_info

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CAP = 8
SNRS = (-12.0, -1.0, 0.0, 0.5, 1.0, 1.5, 3.0, None)          # None: noiseless
BOUND = int(re.search(r"#define LDPC_EAGER_MAX_BAD_LANES (\d+)",
                      (ROOT / "openairinterface5g_amd" / "csrc" / "ldpc_dec_fast_block.h").read_text()).group(1))


def block_llr(rng, BG, Z, R, snr):
    n = O.NCOLS[(BG, R)] * Z
    info = random_info(rng, BG, Z)
    if snr is not None:
        return make_llr(rng, BG, Z, R, snr, info)[:n]
    cw = O.encode(BG, Z, info)[:n - 2 * Z]
    return np.concatenate([np.zeros(2 * Z, np.int8), np.where(cw == 0, 20, -20).astype(np.int8)])


def mixed_batch(BG, Z, R, n, seed, snrs=SNRS):
    """n blocks, the SNRs in turn, with the oracle's pass counts and output rows"""
    rng = np.random.default_rng(seed)
    llr = np.ascontiguousarray(np.stack([block_llr(rng, BG, Z, R, snrs[i % len(snrs)]) for i in range(n)]), np.int8)
    ref = [O.decode(BG, Z, R, llr[i], CAP) for i in range(n)]
    return llr, np.array([r[0] for r in ref], np.int32), np.stack([r[1] for r in ref])


@pytest.mark.parametrize("BG,Z,R", [(1, 384, 13), (2, 208, 15), (1, 64, 13)])
def test_mixed_batch_equals_the_oracle_in_every_launch(hip, BG, Z, R):
    """64 blocks at -12 ... 3 dB and noiseless in one launch: three launches from device memory in the throughput shape (Zc = 384 and
    208: the lifting size's own instantiation; Zc = 64: the general kernel), one in the latency shape and one from host memory"""
    import torch
    llr, its, outs = mixed_batch(BG, Z, R, 64, 5000 + Z)
    assert len(set(its.tolist())) >= 4 and CAP + 1 in its and its.min() <= 3, its.tolist()     # blocks of one launch stop at different passes
    d_llr = torch.from_numpy(llr).cuda()
    results = []
    for kernel in (3, 3, 3, 4):
        d_out = torch.full((64, (outs.shape[1] + 3) // 4 * 4), 0x33, dtype=torch.uint8, device="cuda")
        d_it = torch.full((64,), -7, dtype=torch.int32, device="cuda")
        hip.decode_batch_device(BG, Z, R, d_llr, d_out, d_it, numMaxIter=CAP, kernel=kernel)
        torch.cuda.synchronize()
        results.append((d_it.cpu().numpy(), d_out.cpu().numpy()[:, :outs.shape[1]]))
    results.append(hip.decode_batch_host(BG, Z, R, llr, numMaxIter=CAP))
    for k, (n_iter, out) in enumerate(results):
        assert np.array_equal(n_iter, its), (k, n_iter.tolist(), its.tolist())
        assert np.array_equal(out, outs), k


def test_mixed_blocks_through_the_per_segment_entry_point(hip):
    """the same kinds of block one by one through LDPCdecoder (the resident server's workgroups), three rounds"""
    BG, Z, R = 1, 384, 13
    llr, its, outs = mixed_batch(BG, Z, R, 16, 5100)
    assert CAP + 1 in its and its.min() <= 3 and len(set(its.tolist())) >= 3, its.tolist()
    p = hip.make_dec_params(BG, Z, R, CAP)
    for rnd in range(3):
        for i in range(len(llr)):
            n, out = hip.LDPCdecoder(p, llr[i])
            assert n == its[i] and np.array_equal(out, outs[i]), (rnd, i, n, int(its[i]))


def test_trace_rows_say_where_the_parity_was_skipped(hip, tmp_path):
    """NRLDPC_HIP_DEC_TRACE is read once per process: a child decodes 8 blocks of BG1 Zc = 384 R = 1/3, 4 at -12 dB and 4 at 1 dB,
    through the diagnostic instantiation.  Its rows ([22 + p]: unsatisfied lanes counted by pass p, [32 + p]: tasks of pass p that
    ran without the parity): the -12 dB blocks ran tasks without the parity in every pass from 2 on; no block skipped a task in a
    pass whose count is <= the bound; the results equal the oracle"""
    BG, Z, R = 1, 384, 13
    llr, its, outs = mixed_batch(BG, Z, R, 8, 5200, snrs=(-12.0, 1.0))
    assert (its[0::2] == CAP + 1).all() and (its[1::2] <= CAP).all() and (its[1::2] >= 3).all(), its.tolist()
    np.save(tmp_path / "llr.npy", llr)
    trace = tmp_path / "rows.dectrace"
    env = dict(os.environ, NRLDPC_HIP_DEC_TRACE=str(trace))
    subprocess.run([sys.executable, __file__, str(tmp_path / "llr.npy"), str(tmp_path / "res.npz")], check=True, env=env, timeout=120)
    z = np.load(tmp_path / "res.npz")
    assert np.array_equal(z["n_iter"], its) and np.array_equal(z["out"], outs), z["n_iter"].tolist()
    rows = np.fromfile(trace, dtype=np.uint64).reshape(-1, 32)
    assert rows.shape[0] == 8 and np.array_equal(rows[:, 4].astype(np.int32), its)
    stamps = rows.view(np.uint32).reshape(8, 64)[:, 10:]
    bad, skipped = stamps[:, 23:32].astype(np.int64), stamps[:, 33:42].astype(np.int64)      # passes 1 .. 9
    print("unsatisfied lanes counted by pass 1..9:", bad.tolist(), "tasks without the parity:", skipped.tolist())
    assert (skipped[0::2, 1:] > 0).all(), skipped.tolist()
    assert (skipped[:, 0] == 0).all() and not skipped[bad <= BOUND].any(), (bad.tolist(), skipped.tolist())


if __name__ == "__main__":     # the child of test_trace_rows_say_where_the_parity_was_skipped
    sys.path.insert(0, str(ROOT))
    import openairinterface5g_amd as pkg
    pkg.LDPCinit()
    llr = np.load(sys.argv[1])
    n_iter, out = pkg.decode_batch_host(1, 384, 13, llr, numMaxIter=CAP, kernel=3)
    np.savez(sys.argv[2], n_iter=n_iter, out=out)
