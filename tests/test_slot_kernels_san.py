"""The slot-level kernels on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer, on arrays of exactly the extents
include/nrLDPC_hip.h documents (tests/emul/slot_emul_san.cpp: a stand-alone program over the .hip files themselves, the host shim
and the library's own plans).  A read in front of or behind a caller's array changes no output and passes every canary test on
the GPU; it faults only where the array happens to end with its allocation.  Here it is a report.  The program is built and run
by this test; sanitized code is never loaded into Python.  What the run proves and what it does not: DESIGN.md 4.15."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
EMUL = ROOT / "tests" / "emul"
CSRC = ROOT / "openairinterface5g_amd" / "csrc"
CLANG = "/opt/rocm/lib/llvm/bin/clang"                  # as a plain host compiler: the kernel bodies use clang vector extensions
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g"]
CXXFLAGS = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-pass-failed", "-Wno-unused-function", "-I", str(EMUL / "hip_host"), "-I", str(CSRC)]


def test_slot_kernels_on_exact_buffers_under_the_host_sanitizers(tmp_path):
    # the translation units side by side: most of this test's time is the compiler's
    jobs = [subprocess.Popen([CLANG, *SAN, "-c", str(CSRC / "nr_coding_host.c"), "-o", str(tmp_path / "nr_coding_host.o")])]
    for name in ("slot_emul_san", "slot_rx_emul", "slot_tx_emul", "slot_scr_emul"):
        jobs.append(subprocess.Popen([CLANG + "++", *SAN, *CXXFLAGS, "-c", str(EMUL / (name + ".cpp")), "-o", str(tmp_path / (name + ".o"))]))
    assert [j.wait() for j in jobs] == [0] * len(jobs)
    exe = tmp_path / "slot_emul_san"
    subprocess.run([CLANG + "++", *SAN, "-o", str(exe), *[str(p) for p in sorted(tmp_path.glob("*.o"))], "-lpthread"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-4000:]
    calls, bad = (int(x) for x in r.stdout.split() if x.isdigit())
    assert calls > 1000 and bad == 0, r.stdout
