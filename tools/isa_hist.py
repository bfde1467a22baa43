#!/usr/bin/env python3
"""Static VALU opcode histogram of one kernel in two builds of an object file, priced with the micro-benchmark table (no GPU
needed): the shape of profiles/r07/isa_hist_f16.txt.  A static count: every body weighs one, whatever its share of the tasks.

  python tools/isa_hist.py before.o after.o ['ldpc_dec_fast_kernel<false, false, false, 384>']
"""
import collections
import re
import subprocess
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from valu_issue_model import UBENCH_ROW, ubench_table      # noqa: E402

LLVM = Path("/opt/rocm/lib/llvm/bin")


def histogram(obj, kernel):
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = Path(tmp) / "fat", Path(tmp) / "co"
        subprocess.run([LLVM / "llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
        tgt = [t for t in subprocess.run([LLVM / "clang-offload-bundler", "--type=o", f"--input={fat}", "--list"], check=True,
                                         capture_output=True, text=True).stdout.split() if "gfx950" in t][0]
        subprocess.run([LLVM / "clang-offload-bundler", "--type=o", f"--input={fat}", f"--targets={tgt}", f"--output={co}", "--unbundle"],
                       check=True)
        asm = subprocess.run([LLVM / "llvm-objdump", "-d", "--demangle", co], check=True, capture_output=True, text=True).stdout
    hist, inside = collections.Counter(), False
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            inside = m.group(1).split("(")[0].replace("void ", "").strip() == kernel
            continue
        t = line.split()
        if inside and t and t[0].startswith("v_"):
            hist[t[0]] += 1
    if not hist:
        sys.exit(f"{kernel} not found in {obj}")
    return hist


def main():
    before, after = sys.argv[1], sys.argv[2]
    kernel = sys.argv[3] if len(sys.argv) > 3 else "ldpc_dec_fast_kernel<false, false, false, 384>"
    table = ubench_table()
    hb, ha = histogram(before, kernel), histogram(after, kernel)
    ns = lambda op: table[UBENCH_ROW.get(op.replace("_e32", "").replace("_e64", "").replace("_sdwa", "").replace("_dpp", ""), "xor_b32")]
    print(f"# {kernel}: {before} -> {after}")
    print("%-26s%8s%8s%8s%7s" % ("opcode", "before", "after", "diff", "ns"))
    for op in sorted(set(hb) | set(ha), key=lambda o: -max(hb[o], ha[o])):
        if max(hb[op], ha[op]) >= 50 or hb[op] != ha[op]:
            print("%-26s%8d%8d%+8d%7.2f" % (op, hb[op], ha[op], ha[op] - hb[op], ns(op)))
    tb, ta = sum(hb.values()), sum(ha.values())
    pb, pa = sum(c * ns(o) for o, c in hb.items()), sum(c * ns(o) for o, c in ha.items())
    print("%-26s%8d%8d%+8d" % ("total VALU", tb, ta, ta - tb))
    print("%-26s%8.0f%8.0f%+8.0f   (%+.1f %%)" % ("priced issue time, ns", pb, pa, pa - pb, 100 * (pa - pb) / pb))


if __name__ == "__main__":
    main()
