"""The check-node bodies take a' - r' as one packed f16 subtract that yields sign-magnitude (ldpc_psub_sm).  Host checks:
(a) the host form of ldpc_psub_sm against (0x8000 | a) - r -> (sign, |d|) for all 65 536 byte pairs, in both halves;
(b) every degree the dispatcher serves (3 .. 10 with an extension edge, 8 / 10 / 19 without), first pass and later passes,
    extension LLRs in LDS and in global memory, and the two-minima body in its three modes: the bodies of the tree against a
    verbatim copy of the header before the change (tests/cn_sm/ldpc_dec_fast_core_parent.h) on random LDS images, among them
    images made of the saturation corners 0, 1, 127, 128, 129, 255 only -- identical message bytes (wrap-around pad
    included) and identical return flags.
The degree-19 pair body exists on the device only; the GPU suite checks it against the oracle."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openairinterface5g_amd" / "csrc"
HARNESS = ROOT / "tests" / "cn_sm"
CXX = "/opt/rocm/lib/llvm/bin/clang++"     # the compiler of tests/emul: the bodies use clang vector extensions
# per repetition, corner mode and pass kind: 8 degrees x 2 LLR homes + 3 plain rows through the dispatcher, and per mode of
# the two-minima body 5 x 2 + 2
N_CASES = 8 * 3 * 2 * ((8 * 2 + 3) + 3 * (5 * 2 + 2))


def _run(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.run([CXX, "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-pass-failed", "-I", str(CSRC), "-I", str(HARNESS)]
                   + flags + [str(HARNESS / "cn_sm_harness.cpp"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines()


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("cn_sm")
    return _run(d, "cn_new", []), _run(d, "cn_parent", ["-DCN_PARENT"])


def test_psub_sm_host_form_all_byte_pairs(outputs):
    new, _ = outputs
    assert new[0] == "psub_sm mismatches 0 of 131072"


def test_bodies_match_the_parent_commit(outputs):
    new, parent = outputs
    new = new[1:]
    assert new[-1] == parent[-1] == f"cases {N_CASES}"
    assert len(new) == len(parent) == N_CASES + 1
    diff = [(a, b) for a, b in zip(new, parent) if a != b]
    assert not diff, f"{len(diff)} of {N_CASES} cases differ, first: {diff[0]}"
    # the cases are not trivially equal: message hashes differ from case to case
    assert len({l.split(":")[1] for l in new[:-1]}) == N_CASES
