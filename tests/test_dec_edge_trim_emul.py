"""The fast decoder's node bodies with one instruction less per edge (ldpc_dec_fast_core.h: the bit-node gather sums the odd lanes
as whole words, the check-node output bytes take their sign through two three-input bit operations) against a verbatim copy of the
header before that change (tests/edge_trim/ldpc_dec_fast_core_parent.h), on the host, bit for bit:
  bit nodes   ldpc_fast_bn for column degrees 1 .. 31, the list as long as the column and padded past the next multiple of four
              (both loops of the gather), every byte phase of the shift, every item of the row (the wrap item j = 0 and the last
              one among them), message bytes all 0xff, all 0x01, alternating and random, LLR bytes 0x7f and 0x80, one block and
              several blocks per row (boff_r / boff_a): identical APP dwords, both copies; and the whole-word accumulator, summed
              in 64 bits from the same bytes, stays below 2^32;
  check nodes every degree of ldpc_fast_cn_dispatch and ldpc_fast_cn2_dispatch and the two-minima body in its three modes, first
              pass and later passes, with the parity and without, random images and images of saturated bytes only: identical
              message rows (wrap-around pad included) and identical parity flags.
The harness is a stand-alone program; it is built plain and with -fsanitize=address,undefined and run directly.  The degree-19 pair
body exists on the device only; tests/test_gpu_dec_edge_trim.py checks it against the oracle."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openairinterface5g_amd" / "csrc"
HARNESS = ROOT / "tests" / "edge_trim"
CXX = "/opt/rocm/lib/llvm/bin/clang++"     # the compiler of tests/emul: the bodies use clang vector extensions
# degrees x list lengths x (phases + mixed) x patterns x LLR words, + the several-blocks cases
N_BN = 31 * 2 * 5 * 5 * 3 + 8 * 2 * 2
# per repetition, corner mode, pass kind and parity: 8 degrees x 2 LLR homes + 3 plain rows through the dispatcher, 3 x 2 double
# tasks, and per mode of the two-minima body 3 x 2 + 2
N_CN = 4 * 3 * 2 * 2 * ((8 * 2 + 3) + 3 * 2 + 3 * (3 * 2 + 2))
# 31 edges and the LLR, every byte 0xff: 32 * 255 * (1 + 2^8 + 2^16)
AT_BOUND = 32 * 255 * (1 + 2**8 + 2**16)
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]


def _run(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.run([CXX, "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-pass-failed", "-I", str(CSRC), "-I", str(HARNESS)]
                   + flags + [str(HARNESS / "edge_trim_harness.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (name, r.returncode, r.stderr[-2000:])
    return r.stdout.strip().splitlines()


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("edge_trim")
    return dict(new=_run(d, "new", []), parent=_run(d, "parent", ["-DEDGE_PARENT"]),
                new_san=_run(d, "new_san", SAN), parent_san=_run(d, "parent_san", SAN + ["-DEDGE_PARENT"]))


def _split(lines):
    bn = [l for l in lines if l.startswith("bn deg ")]
    cn = [l for l in lines if l.startswith("cn body ")]
    assert len(bn) + len(cn) + 2 == len(lines)
    return bn, cn


def test_every_case_ran(outputs):
    for name, lines in outputs.items():
        bn, cn = _split(lines)
        assert len(bn) == N_BN and len(cn) == N_CN, (name, len(bn), len(cn))
        assert lines[-1] == f"cn cases {N_CN}" and lines[N_BN].startswith(f"bn cases {N_BN} at_max "), name
    # the sanitizer build computes what the plain build computes
    assert outputs["new"] == outputs["new_san"] and outputs["parent"] == outputs["parent_san"]


def test_bit_node_app_words_match_the_parent(outputs):
    new, parent = _split(outputs["new"])[0], _split(outputs["parent"])[0]
    diff = [(a, b) for a, b in zip(new, parent) if a != b]
    assert not diff, f"{len(diff)} of {N_BN} cases differ, first: {diff[0]}"
    # not trivially equal: random messages give every case its own APP words (the constant patterns saturate alike)
    rand = [re.search(r"app (\w+)", l).group(1) for l in new if " pat 4 " in l]
    assert len(set(rand)) == len(rand) == 31 * 2 * 5 * 3 + 8 * 2


def test_whole_word_accumulator_never_wraps(outputs):
    bn = _split(outputs["new"])[0]
    worst = [int(re.search(r"at_max (\d+) wrapped (\d)", l).group(1)) for l in bn]
    assert not any(l.endswith("wrapped 1") for l in bn)
    # the bound of the comment in ldpc_dec_fast_core.h is reached (degree 31, all bytes 0xff, LLR 0x7f) and not exceeded
    assert max(worst) == AT_BOUND < 2**32
    assert outputs["new"][N_BN] == f"bn cases {N_BN} at_max {AT_BOUND}"


def test_check_node_rows_and_flags_match_the_parent(outputs):
    new, parent = _split(outputs["new"])[1], _split(outputs["parent"])[1]
    diff = [(a, b) for a, b in zip(new, parent) if a != b]
    assert not diff, f"{len(diff)} of {N_CN} cases differ, first: {diff[0]}"
    # not trivially equal: on the random images the message hashes differ from case to case (saturated bytes leave most minima 0)
    rand = [l.split(":")[1].split()[1] for l in new if l.split(":")[0].endswith("corners 0 ")]
    assert len(set(rand)) == len(rand) == N_CN // 3
