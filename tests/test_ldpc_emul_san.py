"""The decoder's, the encoders' and the chain phases' per-thread code on the CPU (tests/emul/ldpc_emul.cpp, tb_rx_scr_emul.cpp,
tb_rx_sym_emul.cpp, tb_tx_scr_emul.cpp, tb_tx_sym_emul.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer, with inputs and outputs of exactly the documented
extents and the oracle's C sources in the same program (tests/emul/ldpc_emul_san.cpp, a stand-alone program: sanitized code is
never loaded into Python).  The emulator's own arrays carry no slack: the LDS images are as large as the kernels ask for, the
input copy is num_llr bytes in whole words, the encoders' scratch is what the headers document.  A gate for the next decoder
change; what a clean run proves and what it does not: DESIGN.md 4.15."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
EMUL = ROOT / "tests" / "emul"
CSRC = ROOT / "openairinterface5g_amd" / "csrc"
ORACLE = ROOT / "oracle"
CLANG = "/opt/rocm/lib/llvm/bin/clang"                  # as a plain host compiler: the kernel bodies use clang vector extensions
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g"]


def test_decoder_and_encoders_on_exact_buffers_under_the_host_sanitizers(tmp_path):
    # the translation units side by side: most of this test's time is the compiler's
    jobs = [subprocess.Popen([CLANG, *SAN, "-std=gnu11", "-c", str(src), "-o", str(tmp_path / (src.stem + ".o"))])
            for src in (CSRC / "ldpc_graph.c", CSRC / "nr_coding_host.c", ORACLE / "oracle_ldpc_decoder.c", ORACLE / "oracle_ldpc_encoder.c",
                        ORACLE / "oracle_crc_seg_rm.c")]
    jobs += [subprocess.Popen([CLANG + "++", *SAN, "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-pass-failed", "-I", str(CSRC), "-c",
                               str(EMUL / (name + ".cpp")), "-o", str(tmp_path / (name + ".o"))])
             for name in ("ldpc_emul", "tb_rx_scr_emul", "tb_rx_sym_emul", "tb_tx_scr_emul", "tb_tx_sym_emul", "ldpc_emul_san")]
    assert [j.wait() for j in jobs] == [0] * len(jobs)
    exe = tmp_path / "ldpc_emul_san"
    subprocess.run([CLANG + "++", *SAN, "-o", str(exe), *[str(p) for p in sorted(tmp_path.glob("*.o"))], "-lm", "-lpthread"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-4000:]
    calls, bad = (int(x) for x in r.stdout.split() if x.isdigit())
    assert calls > 8000 and bad == 0, r.stdout
