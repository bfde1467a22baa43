"""The dump file of the C harnesses (tests/abi_cases.h): the calls a harness compares everything else with, read back and
held against the oracle on the same inputs -- what the threads of abi_threads.c / abi_lifecycle.c agree with is then the
oracle's answer, not merely the library's own first one."""
import numpy as np

import oracle_lib as O

MAGIC = 0x41424944
FIELDS = ("magic", "kind", "BG", "Z", "R", "max_iter", "use_crc", "E", "crc_type", "out_init", "n_iter", "in_len", "out_len")


def read(path):
    """list of dict(FIELDS..., inp=int8/uint8 array, out=uint8 array); R holds Kb for encoder records (kind 1)"""
    raw = np.fromfile(path, dtype=np.uint8)
    recs, pos = [], 0
    while pos < raw.size:
        h = raw[pos:pos + 64].view(np.int32)
        assert h.size == 16 and h[0] == MAGIC, (path, pos)
        r = dict(zip(FIELDS, (int(x) for x in h)))
        pos += 64
        r["inp"] = raw[pos:pos + r["in_len"]].copy()
        pos += r["in_len"]
        r["out"] = raw[pos:pos + r["out_len"]].copy()
        pos += r["out_len"]
        assert r["inp"].size == r["in_len"] and r["out"].size == r["out_len"], (path, "truncated")
        recs.append(r)
    return recs


def check_against_oracle(path, n_dec, n_enc=0):
    """every record of the dump equals the oracle on the dumped inputs: pass counts and bytes; returns the pass counts"""
    recs = read(path)
    assert [r["kind"] for r in recs] == [0] * n_dec + [1] * n_enc, [r["kind"] for r in recs]
    iters = []
    for i, r in enumerate(recs):
        BG, Z = r["BG"], r["Z"]
        if r["kind"] == 0:
            llr = r["inp"].view(np.int8)
            assert llr.size == O.NCOLS[(BG, r["R"])] * Z
            n_ref, out_ref = O.decode(BG, Z, r["R"], llr, r["max_iter"], O.OUT_BIT, bool(r["use_crc"]), r["E"], r["crc_type"],
                                      out_init=r["out_init"])
            assert r["n_iter"] == n_ref and np.array_equal(r["out"], out_ref), ("decoder record", i, BG, Z, r["R"], r["n_iter"], n_ref)
            iters.append(n_ref)
        else:
            ref = O.encode(BG, Z, r["inp"], r["R"])
            assert r["out_len"] == ref.size and np.array_equal(r["out"], ref), ("encoder record", i, BG, Z)
    return iters
