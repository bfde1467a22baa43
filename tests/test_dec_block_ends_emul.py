"""What the fast decoder's block body does outside its passes -- the prologue with the LLR extents from the kernel arguments and its
LLR loads made unconditionally, the hard decision, the request for the next block's row (ldpc_dec_fast_block.h; the request is an
A/B arm, -DLDPC_DEC_WARM=1, off by default) -- on the CPU as written, against the oracle.

tests/dec_block_ends/dec_block_ends_harness.cpp is a stand-alone program over ldpc_decoder_fast.hip itself and the host shim of
tests/emul/hip_host.  It is built plain, as the library is, and with -fsanitize=address,undefined and the request compiled in, and
run directly, never loaded into Python.  Per code (dec_block_ends_inputs.CODES: ncore Z no multiple of 64 or of 32, lifting sizes
that divide no power of two, one that is 64, the Zc = 384 instantiation at both ends of its rates) one launch of three blocks -- the
oracle's pass counts 3, 4 and numMaxIter + 1 -- with warm_ahead = 1: the requested row lies inside the batch for blocks 0 and 1 (the
last row for block 1) and past its end for block 2, and the LLR array ends with the last row, so a request or a prologue load past
the end is a sanitizer report.  Checked: every output row byte for byte (the zero words behind ncore Z among them), the 0xAA guard
bytes on both sides of every row (rows 8 bytes apart: with an odd dword count every other row is only 4-byte aligned), the pass
counts, and that the sanitized build prints what the plain one prints."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from dec_block_ends_inputs import CAP, CODES, WANTED, stop_rows

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openairinterface5g_amd" / "csrc"
EMUL = ROOT / "tests" / "emul"
HARNESS = ROOT / "tests" / "dec_block_ends" / "dec_block_ends_harness.cpp"
CLANG = "/opt/rocm/lib/llvm/bin/clang"      # the compiler of tests/emul: the bodies use clang vector extensions
FLAGS = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-pass-failed", "-Wno-unused-function", "-I", str(EMUL / "hip_host"), "-I", str(EMUL),
         "-I", str(CSRC), "-DLDPC_FAST_ZC_LIST(X)=X(384)"]       # one lifting size's own instantiations: the one the cases run
BUILDS = {"plain": ["-O2"], "san": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DLDPC_DEC_WARM=1"]}


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("dec_block_ends")
    jobs = []
    for name, flags in BUILDS.items():
        jobs.append(subprocess.Popen([CLANG, *flags, "-c", str(CSRC / "ldpc_graph.c"), "-o", str(d / f"graph_{name}.o")]))
        jobs.append(subprocess.Popen([CLANG + "++", *flags, *FLAGS, "-c", str(HARNESS), "-o", str(d / f"harness_{name}.o")]))
    assert [j.wait() for j in jobs] == [0] * len(jobs)
    for name, flags in BUILDS.items():
        subprocess.run([CLANG + "++", *flags, "-o", str(d / name), str(d / f"harness_{name}.o"), str(d / f"graph_{name}.o"), "-lpthread"], check=True)
    return d


def run(programs, build, BG, Z, R, llr, warm):
    f = programs / f"llr_{BG}_{Z}_{R}.bin"
    llr.tofile(f)
    r = subprocess.run([str(programs / build), str(BG), str(Z), str(R), str(len(llr)), str(CAP), str(warm), str(f)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and r.stderr == "", (build, BG, Z, R, r.returncode, r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("BG,Z,R", CODES)
def test_rows_guards_and_pass_counts(programs, BG, Z, R):
    llr, its, outs = stop_rows(BG, Z, R)
    assert its.tolist() == list(WANTED)
    text = run(programs, "plain", BG, Z, R, llr, warm=1)
    info, it_line, out_line = text.strip().splitlines()
    num_llr, ob, pitch = (int(x) for x in info.split()[1:4])
    assert num_llr == llr.shape[1] and ob == outs.shape[1] and pitch == ob + 8
    print(BG, Z, R, info, it_line)
    assert [int(x) for x in it_line.split()[1:]] == its.tolist()
    buf = np.frombuffer(bytes.fromhex(out_line.split()[1]), np.uint8)
    assert len(buf) == 4 + len(llr) * pitch
    assert (buf[:4] == 0xAA).all()
    for b in range(len(llr)):
        row = buf[4 + b * pitch:4 + (b + 1) * pitch]
        assert np.array_equal(row[:ob], outs[b]), (b, np.flatnonzero(row[:ob] != outs[b])[:8].tolist())
        assert (row[ob:] == 0xAA).all(), (b, row[ob:].tolist())
    # the cases are what the module says they are: a last 64-bit group that is partial, groups across column ends, zero words behind the bits
    ncz = (26 if BG == 1 else 14) * Z
    if Z == 8:
        assert ncz % 64 != 0
    if Z in (12, 20):
        assert 64 % Z != 0 and Z % 64 != 0
    assert not outs[:, (ncz + 7) // 8:].any() and outs[:2, :ncz // 8].any()
    # the same under AddressSanitizer and UndefinedBehaviorSanitizer: nothing reported, the same bytes
    assert run(programs, "san", BG, Z, R, llr, warm=1) == text


def test_warming_switched_off_and_past_the_end_change_nothing(programs):
    """The build with the request compiled in: warm_ahead = 0 (nothing requested), 2 (block 0 asks for the last row, the others are
    past the end) and 3 (the first index past the end): the same rows, nothing reported."""
    BG, Z, R = CODES[2]
    llr, _, _ = stop_rows(BG, Z, R)
    texts = {w: run(programs, "san", BG, Z, R, llr, warm=w) for w in (0, 1, 2, 3)}
    assert len(set(texts.values())) == 1
