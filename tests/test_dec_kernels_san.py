"""The decoder kernels on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer, on arrays of exactly the documented extents
(tests/emul/dec_emul_san.cpp: a stand-alone program over ldpc_decoder.hip, ldpc_decoder_fast.hip and tb_rx_fused.hip themselves and the
host shim):
num_llr input bytes per block, out_bytes per output row, a workgroup's LDS exactly as long as its launch asks for.  A read behind
a block's last LLR or behind the LDS a descriptor reserves changes no result and passes every test on the GPU; here it is a
report.  The program is built and run by this test; sanitized code is never loaded into Python.  What the run proves and what it
does not: DESIGN.md 4.16."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
EMUL = ROOT / "tests" / "emul"
CSRC = ROOT / "openairinterface5g_amd" / "csrc"
CLANG = "/opt/rocm/lib/llvm/bin/clang"                  # as a plain host compiler: the kernel bodies use clang vector extensions
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O0", "-g"]    # -O0: see dec_emul_san.cpp
CXXFLAGS = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-pass-failed", "-Wno-unused-function", "-I", str(EMUL / "hip_host"), "-I", str(CSRC),
            "-DLDPC_FAST_ZC_LIST(X)=X(208)"]            # one lifting size's own instantiations: see dec_emul_san.cpp


def test_decoder_kernels_on_exact_buffers_under_the_host_sanitizers(tmp_path):
    # the translation units side by side: most of this test's time is the compiler's
    jobs = [subprocess.Popen([CLANG, *SAN, "-c", str(CSRC / (name + ".c")), "-o", str(tmp_path / (name + ".o"))]) for name in ("ldpc_graph", "nr_coding_host")]
    for name in ("dec_emul_san", "dec_fast_emul", "rx_fused_emul"):
        jobs.append(subprocess.Popen([CLANG + "++", *SAN, *CXXFLAGS, "-c", str(EMUL / (name + ".cpp")), "-o", str(tmp_path / (name + ".o"))]))
    assert [j.wait() for j in jobs] == [0] * len(jobs)
    exe = tmp_path / "dec_emul_san"
    subprocess.run([CLANG + "++", *SAN, "-o", str(exe), *[str(p) for p in sorted(tmp_path.glob("*.o"))], "-lpthread"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-4000:]
    calls, bad = (int(x) for x in r.stdout.split() if x.isdigit())
    assert calls >= 22 and bad == 0, r.stdout
