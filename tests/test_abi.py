"""The C-ABI shared library (CPU only, no compute): it loads, exports every function include/*.h declares, and the
parameter structures have the layout the reference's callers use."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def declared_functions():
    txt = (ROOT / "include" / "nrLDPC_hip.h").read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = re.findall(r"^\s*(?:const\s+)?(?:int32_t|uint32_t|int|char|void)\s*\*?\s*(\w+)\s*\(", txt, flags=re.M)
    return sorted(set(names))


def test_library_exports_every_declared_symbol(built):
    import openairinterface5g_amd as pkg
    L = pkg.load_library()
    names = declared_functions()
    assert {"LDPCinit", "LDPCshutdown", "LDPCdecoder", "LDPCencoder", "LDPCdecoder_batch", "LDPCencoder_batch"} <= set(names)
    for n in names:
        assert getattr(L, n) is not None, n
    assert sorted(pkg.ldpc.EXPORTS) == names
    # the reference's loader resolves exactly these four by name (nrLDPC_load.c:55-65)
    out = subprocess.run(["nm", "-D", "--defined-only", str(pkg.ldpc.LIB_PATH)], capture_output=True, text=True).stdout
    for n in ("LDPCinit", "LDPCshutdown", "LDPCdecoder", "LDPCencoder"):
        assert re.search(rf"\bT {n}$", out, flags=re.M), n
    # nothing but the declared functions is visible: OAI loads plugins RTLD_GLOBAL (load_module_shlib.c:160), helper names
    # (graph builders, kernel launchers, host-side segmentation helpers) must not land in the executable's namespace
    exported = sorted(l.split()[-1] for l in out.splitlines() if l.split()[1:2] and l.split()[1] in "TDBR")
    assert exported == names, sorted(set(exported) ^ set(names))
    # ... and the replacement must not need host-executable symbols the way the reference .so does
    und = subprocess.run(["nm", "-D", "--undefined-only", str(pkg.ldpc.LIB_PATH)], capture_output=True, text=True).stdout
    for bad in ("g_log", "logRecord_mt", "exit_function", "opp_enabled"):
        assert bad not in und


def test_offload_slot_library_exports_the_plugin_symbols(built):
    """libldpc_hip_t2.so, the personality of the reference's second plugin slot (nr_init.c:138-139): exactly the four names
    load_LDPClib resolves plus the version hook; it needs libldpc_hip.so (found beside it) and nothing of the executable."""
    import openairinterface5g_amd as pkg
    t2 = Path(pkg.ldpc.LIB_PATH).parent / "libldpc_hip_t2.so"
    out = subprocess.run(["nm", "-D", "--defined-only", str(t2)], capture_output=True, text=True).stdout
    exported = sorted(l.split()[-1] for l in out.splitlines() if l.split()[1:2] and l.split()[1] in "TDBR")
    assert exported == sorted(pkg.ldpc.T2_EXPORTS)
    dyn = subprocess.run(["readelf", "-d", str(t2)], capture_output=True, text=True).stdout
    assert "libldpc_hip.so" in dyn and "$ORIGIN" in dyn
    und = subprocess.run(["nm", "-D", "--undefined-only", str(t2)], capture_output=True, text=True).stdout
    assert {"nrLDPC_hip_offload_decoder", "nrLDPC_hip_offload_encoder", "nrLDPC_hip_offload_init"} <= set(und.split())
    for bad in ("g_log", "logRecord_mt", "exit_function", "opp_enabled", "rte_"):
        assert bad not in und
    L = C.CDLL(str(t2))                     # loads (and pulls libldpc_hip.so in) without a GPU; LDPCinit is what needs one
    for n in pkg.ldpc.T2_EXPORTS:
        assert getattr(L, n) is not None


def test_loader_version_hook(built):
    """ldpc_checkbuildver, the hook load_module_version_shlib() calls after dlopen (load_module_shlib.c:174-185): reports
    the library's build string; NRLDPC_HIP_REQUIRE_BUILD turns a foreign executable into a load-time refusal."""
    import os
    import sys
    code = ("import ctypes as C, sys; sys.path.insert(0, %r); import openairinterface5g_amd as p; L = p.load_library();"
            "v = C.c_char_p(); L.ldpc_checkbuildver.argtypes = [C.c_char_p, C.POINTER(C.c_char_p)];"
            "rc = L.ldpc_checkbuildver(b'Branch: develop Abrev. Hash: 0123abc Date: x', C.byref(v)); print(rc, v.value.decode())" % str(ROOT))
    for need, rc in ((None, 0), ("0123abc", 0), ("Hash: ffff", -1)):
        env = {k: v for k, v in os.environ.items() if k != "NRLDPC_HIP_REQUIRE_BUILD"}
        if need:
            env["NRLDPC_HIP_REQUIRE_BUILD"] = need
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert r.stdout.split()[0] == str(rc) and "libldpc_hip" in r.stdout and "gfx950" in r.stdout, (need, r.stdout, r.stderr)


def test_loader_autoinit_hook(built):
    """ldpc_autoinit, the loader's second optional hook (load_module_shlib.c:186-191): NULL -- what load_LDPClib passes
    (nrLDPC_load.c:61) -- is a no-op; a GPU list goes into NRLDPC_HIP_DEVICES unless the variable is set; anything else is refused."""
    import os
    import sys
    code = ("import ctypes as C, os, sys; sys.path.insert(0, %r); import openairinterface5g_amd as p; L = p.load_library();"
            "L.ldpc_autoinit.argtypes = [C.c_void_p]; libc = C.CDLL(None); libc.getenv.restype = C.c_char_p;"
            "a = L.ldpc_autoinit(None); e0 = libc.getenv(b'NRLDPC_HIP_DEVICES');"
            "s = C.create_string_buffer(b'2,3'); b = L.ldpc_autoinit(C.cast(s, C.c_void_p)); e1 = libc.getenv(b'NRLDPC_HIP_DEVICES');"
            "t = C.create_string_buffer(b'5'); c = L.ldpc_autoinit(C.cast(t, C.c_void_p)); e2 = libc.getenv(b'NRLDPC_HIP_DEVICES');"
            "u = C.create_string_buffer(b'gpu0'); d = L.ldpc_autoinit(C.cast(u, C.c_void_p));"
            "print(a, e0, b, e1, c, e2, d)" % str(ROOT))
    env = {k: v for k, v in os.environ.items() if k != "NRLDPC_HIP_DEVICES"}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert r.stdout.split() == ["0", "None", "0", "b'2,3'", "0", "b'2,3'", "-1"], (r.stdout, r.stderr)


def test_introspection_without_gpu(built):
    import openairinterface5g_amd as pkg
    L = pkg.load_library()
    assert L.nrLDPC_hip_num_llr(1, 384, 13) == 68 * 384 and L.nrLDPC_hip_num_llr(2, 64, 23) == 17 * 64
    assert L.nrLDPC_hip_num_llr(1, 17, 13) == -1 and L.nrLDPC_hip_num_llr(1, 16, 15) == -1
    assert L.nrLDPC_hip_out_bytes(1, 384, 13, 0) == 3264 and L.nrLDPC_hip_out_bytes(1, 2, 13, 0) == 20
    assert 0 < L.nrLDPC_hip_lds_bytes(1, 384, 13) <= 160 * 1024
    assert b"gfx950" in L.nrLDPC_hip_version()


def test_every_code_with_zc_multiple_of_four_keeps_its_fast_descriptor(built):
    """The fast kernel's descriptor builder gives up silently (-> generic kernel) when a table does not fit; no (BG, Zc, R)
    with Zc % 4 == 0, Zc >= 8 may do that (column lists are padded for the interleaved bit-node walk, ldpc_graph.h)."""
    import openairinterface5g_amd as pkg
    sizes = [a * 2 ** j for a in (2, 3, 5, 7, 9, 11, 13, 15) for j in range(8) if a * 2 ** j <= 384]
    assert len(sizes) == 51
    n = 0
    for BG, rates in ((1, (13, 23, 89)), (2, (15, 13, 23))):
        for Z in sizes:
            for R in rates:
                info = pkg.ldpc.code_info(BG, Z, R)
                if Z % 4 == 0 and Z >= 8:
                    n += 1
                    assert info["kernel"] == "fast", (BG, Z, R, info)
    assert n == 210


def test_struct_layouts_match_the_c_header(built, tmp_path):
    """ctypes mirrors (used by every Python-side test) vs the compiler's view of include/nrLDPC_hip.h."""
    import openairinterface5g_amd as pkg
    src = tmp_path / "lay.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "nrLDPC_hip.h"
#define P(T, F) printf(#T "." #F " %zu\n", offsetof(T, F))
int main(void) {
  printf("t_nrLDPC_dec_params %zu\n", sizeof(t_nrLDPC_dec_params));
  P(t_nrLDPC_dec_params, Z); P(t_nrLDPC_dec_params, R); P(t_nrLDPC_dec_params, numMaxIter); P(t_nrLDPC_dec_params, E);
  P(t_nrLDPC_dec_params, outMode); P(t_nrLDPC_dec_params, crc_type); P(t_nrLDPC_dec_params, check_crc); P(t_nrLDPC_dec_params, setCombIn);
  printf("encoder_implemparams_t %zu\n", sizeof(encoder_implemparams_t));
  P(encoder_implemparams_t, Kr); P(encoder_implemparams_t, Kb); P(encoder_implemparams_t, Zc); P(encoder_implemparams_t, BG);
  P(encoder_implemparams_t, K); P(encoder_implemparams_t, F); P(encoder_implemparams_t, E); P(encoder_implemparams_t, rv);
  printf("decode_abort_t %zu\n", sizeof(decode_abort_t)); P(decode_abort_t, failed);
  printf("nrLDPC_hip_dec_batch_t %zu\n", sizeof(nrLDPC_hip_dec_batch_t));
  P(nrLDPC_hip_dec_batch_t, n_blocks); P(nrLDPC_hip_dec_batch_t, llr); P(nrLDPC_hip_dec_batch_t, out_stride);
  P(nrLDPC_hip_dec_batch_t, n_iter); P(nrLDPC_hip_dec_batch_t, mem); P(nrLDPC_hip_dec_batch_t, stream); P(nrLDPC_hip_dec_batch_t, kernel);
  printf("nrLDPC_hip_enc_batch_t %zu\n", sizeof(nrLDPC_hip_enc_batch_t));
  P(nrLDPC_hip_enc_batch_t, Zc); P(nrLDPC_hip_enc_batch_t, Kb); P(nrLDPC_hip_enc_batch_t, in); P(nrLDPC_hip_enc_batch_t, out_stride); P(nrLDPC_hip_enc_batch_t, stream);
  return 0; }''')
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.strip().splitlines())
    m = pkg.ldpc
    py = {"t_nrLDPC_dec_params": m.t_nrLDPC_dec_params, "encoder_implemparams_t": m.encoder_implemparams_t,
          "decode_abort_t": m.decode_abort_t, "nrLDPC_hip_dec_batch_t": m.nrLDPC_hip_dec_batch_t,
          "nrLDPC_hip_enc_batch_t": m.nrLDPC_hip_enc_batch_t}
    for key, val in got.items():
        if "." in key:
            t, f = key.split(".")
            f = {"in": "in_"}.get(f, f)
            assert getattr(py[t], f).offset == int(val), key
        else:
            assert C.sizeof(py[key]) == int(val), key
    # layout the reference's callers compile against (nrLDPC_types.h:84-97 on x86-64): 40 bytes, check_crc at 24
    assert got["t_nrLDPC_dec_params"] == "40" and got["t_nrLDPC_dec_params.check_crc"] == "24"


REF = Path("/root/reference")
REF_LAYOUTS = ROOT / "tests" / "golden" / "ref_abi_layouts.json"


def reference_layouts(tmp_path):
    """What the reference's own headers print through tests/abi_offsets.c and the encoder / abort-struct program below
    (needs the reference tree): {"abi_offsets": text, "enc_fields": [field names], "enc_layout": text}."""
    inc = ["-I", str(REF / "openair1"), "-I", str(REF / "common" / "utils"), "-I", str(REF)]
    exe = tmp_path / "abi_ref"
    subprocess.run(["gcc", "-DUSE_REFERENCE"] + inc + [str(ROOT / "tests" / "abi_offsets.c"), "-o", str(exe)], check=True)
    offsets = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout

    def typedef_text(path, name):
        txt = (REF / path).read_text()
        end = txt.index("} %s;" % name)
        start = txt.rindex("typedef struct", 0, end)
        return txt[start:end + len("} %s;" % name)]

    enc = typedef_text("openair1/PHY/CODING/nrLDPC_defs.h", "encoder_implemparams_t")
    ab = typedef_text("openair1/PHY/defs_common.h", "decode_abort_t")
    fields_enc = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/|//[^\n]*", "", enc[enc.index("{") + 1:enc.rindex("}")], flags=re.S))
    src = tmp_path / "enc_ref.c"
    src.write_text(_ENC_PROG % ('#include "PHY/CODING/nrLDPC_decoder/nrLDPC_types.h"', enc, ab, _enc_body(fields_enc)))
    exe = tmp_path / "enc_ref"
    subprocess.run(["gcc"] + inc + [str(src), "-o", str(exe)], check=True)
    layout = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return {"abi_offsets": offsets, "enc_fields": fields_enc, "enc_layout": layout}


_ENC_PROG = ("#include <stddef.h>\n#include <stdio.h>\n#include <stdbool.h>\n#include <pthread.h>\n%s\n%s\n%s\n"
             "#define F(T, f) printf(#T \".\" #f \" %%zu %%zu\\n\", offsetof(T, f), sizeof(((T *)0)->f))\n"
             "int main(void) { printf(\"%%zu %%zu\\n\", sizeof(encoder_implemparams_t), sizeof(decode_abort_t)); %s F(decode_abort_t, mutex_failure); F(decode_abort_t, failed); return 0; }\n")


def _enc_body(fields):
    return " ".join("F(encoder_implemparams_t, %s);" % f for f in fields)


def test_layouts_against_the_reference_headers(built, tmp_path):
    """The plugin ABI structures as the REFERENCE's own headers declare them vs include/nrLDPC_hip.h, compiler against
    compiler.  nrLDPC_decoder/nrLDPC_types.h (t_nrLDPC_dec_params, e_nrLDPC_outMode, t_nrLDPC_time_stats, time_stats_t via
    common/utils/time_meas.h) compiles on its own: tests/abi_offsets.c is built once against it and once against our
    header and the printed sizes / offsets / enum values must be identical.  encoder_implemparams_t (nrLDPC_defs.h:40-66)
    and decode_abort_t (defs_common.h:998-1001) sit in headers that pull in the un-vendored SIMDE: their typedef TEXT is
    read from the reference (nothing of it is copied into the repository) and compiled next to nrLDPC_types.h.
    What the reference's side prints travels as tests/golden/ref_abi_layouts.json (tools/make_ref_abi_fixture.py); where
    the reference tree is readable it is compiled again and must print exactly that."""
    import json
    import ref_lib as RL
    want = json.loads(REF_LAYOUTS.read_text())
    if RL.readable(REF / "openair1" / "PHY" / "CODING" / "nrLDPC_defs.h"):
        assert reference_layouts(tmp_path) == want
    exe = tmp_path / "abi_ours"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(ROOT / "tests" / "abi_offsets.c"), "-o", str(exe)], check=True)
    ours = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    assert want["abi_offsets"] == ours and ours.count("\n") >= 30, (want["abi_offsets"], ours)
    src = tmp_path / "enc_ours.c"
    src.write_text(_ENC_PROG % ('#include "nrLDPC_hip.h"', "", "", _enc_body(want["enc_fields"])))
    exe = tmp_path / "enc_ours"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    assert want["enc_layout"] == res and len(want["enc_fields"]) >= 19, (want["enc_layout"], res)


def test_no_cpu_fallback_without_gpu(built):
    """On a machine without a HIP device every entry point must fail loudly (this container); on the GPU box the
    call simply succeeds."""
    import numpy as np
    import openairinterface5g_amd as pkg
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        pkg.LDPCinit()
        return
    with pytest.raises(RuntimeError, match="no HIP device"):
        pkg.LDPCinit()
    with pytest.raises(RuntimeError, match="no HIP device"):
        pkg.decode_batch_host(1, 16, 13, np.zeros((1, 68 * 16), np.int8))
    with pytest.raises(RuntimeError, match="no HIP device"):
        pkg.encode_batch_host(1, 16, np.zeros((1, 44), np.uint8))
