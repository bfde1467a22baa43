"""csrc/job_layout.h, the layout of the transport-block calls' job buffers, alone on the CPU: tests/job_layout_check.cpp (its own
main) builds seeded random layouts -- copied parts of 4 / 8 / 12 / 24 / 48-byte elements, zero parts, reserved parts, empty ones of
each kind -- and checks offsets against the plain align_up chain, copied parts byte for byte, zero parts, and a canary behind
upload_bytes().  No GPU."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("job_layout") / "job_layout_check"
    subprocess.run([CXX, "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", str(ROOT / "openairinterface5g_amd" / "csrc"), "-o", str(exe),
                    str(ROOT / "tests" / "job_layout_check.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", [1, 20261018])
def test_random_layouts_against_the_align_up_chain(check, seed):
    r = subprocess.run([str(check), str(seed), "400"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    n = {k: [int(x) for x in v.split(",")] for k, v in re.findall(r"(\w+)=([\d,]+)", r.stdout)}
    assert n["rounds"] == [400]
    # the run held every kind of part, empty ones of every kind, and every element size
    for k in ("copied", "zeros", "reserved", "empty_copied", "empty_zeros", "empty_reserved"):
        assert n[k][0] > 20, (k, r.stdout)
    assert len(n["sizes"]) == 5 and min(n["sizes"]) > 20, r.stdout
