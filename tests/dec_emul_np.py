"""tests/emul/libdec_emul.so from Python: the decoder .hip files themselves run on the CPU (tests/emul/dec_fast_emul.cpp), one real
thread per work-item.  Shared by tests/test_dec_kernels_emul.py and, run as a script, by its child processes -- a switch the
library reads once per process (NRLDPC_HIP_ZC) can only be turned in a fresh one:

    python dec_emul_np.py <in.npz> <out.npz>     in: p (the int32 parameters), llr [n, num_llr]; out: rc, n_iter, out, takes_zc
"""
import ctypes as C
import functools
import re
import sys
from pathlib import Path

import numpy as np

EMUL = Path(__file__).resolve().parent / "emul"
KERNEL_FAST, KERNEL_MULTI, KERNEL_PULL, KERNEL_GENERIC = 0, 1, 2, 3
OUT_INIT = 0x3C


@functools.lru_cache(maxsize=None)
def names(prefix):
    """the enumerators DEC_<prefix>_* (or <prefix>_* for a prefix with an underscore, as RXF_T) of tests/emul/dec_emul_common.h
    in their order (the last one is the count)"""
    text = (EMUL / "dec_emul_common.h").read_text()
    found = []
    for m in re.finditer(r"\b%s_([A-Z0-9_]+)\b" % (prefix if "_" in prefix else "DEC_" + prefix), text):
        if m.group(1) not in found:
            found.append(m.group(1))
    assert found[-1] == "COUNT"
    return {n: i for i, n in enumerate(found)}


@functools.lru_cache(maxsize=None)
def lib():
    L = C.CDLL(str(EMUL / "libdec_emul.so"))
    L.dec_emul_fast_info.argtypes = [C.c_int] * 6 + [C.c_void_p]
    L.dec_emul_takes_zc_kernel.argtypes = [C.c_int] * 4
    L.dec_emul_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.dec_emul_decode_jobs.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p] * 4
    return L


HARQ_STRIDE = 66 * 384          # int16 per soft-buffer row, as the library's callers lay them


def fused_run(tbs, llrs, harq, gen, cap=8, want_rows=False, **options):
    """One launch of the fused UL segment kernel over the transport blocks tbs (dicts A, G, BG, Qm, Nl, rv, round, tbslbrm,
    llrLen [updated], c_init) with their LLR arrays llrs; harq [total segments, HARQ_STRIDE] int16 and gen [len(tbs)] uint32 are
    updated in place.  Returns dict(rc, payload [list per block], ack, iter_max, seg [n_seg, fields], info, rows)."""
    T, Oo, I, S = names("RXF_T"), names("RXF_O"), names("RXF_I"), names("RXF_S")
    L = lib()
    L.rx_fused_emul_run.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 8 + [C.c_uint32, C.c_void_p]
    tb = np.zeros((len(tbs), T["COUNT"]), np.int32)
    for i, t in enumerate(tbs):
        for k, f in (("A", "A"), ("G", "G"), ("BG", "BG"), ("QM", "Qm"), ("NL", "Nl"), ("RV", "rv"), ("ROUND", "round"), ("TBSLBRM", "tbslbrm")):
            tb[i, T[k]] = t[f]
        tb[i, T["MAX_ITER"]] = cap
        tb[i, T["LLRLEN"]] = t.get("llrLen", 0)
        tb[i, T["C_INIT"]] = t.get("c_init", 0)
    opt = np.zeros(Oo["COUNT"], np.int32)
    for k, v in dict(dict(trunc=1, abort=1, mute=1), **options).items():
        opt[Oo[k.upper()]] = int(v)
    llr = np.ascontiguousarray(np.concatenate(llrs), np.int16)
    assert harq.dtype == np.int16 and harq.flags.c_contiguous and harq.shape[1] == HARQ_STRIDE
    pay = np.full(sum(t["A"] // 8 for t in tbs), 0xA5, np.uint8)
    ack = np.full(len(tbs), 7, np.uint8)
    itm = np.full(len(tbs), -7, np.int32)
    seg = np.zeros((harq.shape[0], S["COUNT"]), np.int32)
    inf = np.zeros(I["COUNT"], np.int32)
    l_stride = 68 * 384
    rows = np.full((harq.shape[0], l_stride), 0x11, np.int8) if want_rows else None
    rc = L.rx_fused_emul_run(len(tbs), tb.ctypes.data, opt.ctypes.data, HARQ_STRIDE, llr.ctypes.data, harq.ctypes.data, pay.ctypes.data,
                             ack.ctypes.data, itm.ctypes.data, gen.ctypes.data, seg.ctypes.data,
                             None if rows is None else rows.ctypes.data, l_stride, inf.ctypes.data)
    for i, t in enumerate(tbs):
        t["llrLen"] = int(tb[i, T["LLRLEN"]])
    off = np.cumsum([0] + [t["A"] // 8 for t in tbs])
    return dict(rc=rc, payload=[pay[off[i]:off[i + 1]] for i in range(len(tbs))], ack=ack, iter_max=itm,
                seg={k: seg[:, i] for k, i in S.items() if k != "COUNT"}, info={k: int(inf[i]) for k, i in I.items() if k != "COUNT"},
                rows=rows)


def info(kernel, BG, Z, R, shape=0, mb=0):
    """what the descriptor of a launch says (None: the builder refuses the code)"""
    I = names("I")
    a = np.zeros(I["COUNT"], np.int32)
    if lib().dec_emul_fast_info(kernel, BG, Z, R, shape, mb, a.ctypes.data) != 0:
        return None
    return {k: int(a[i]) for k, i in I.items() if k != "COUNT"}


def params(**kw):
    P = names("P")
    p = np.zeros(P["COUNT"], np.int32)
    p[P["ZC"]] = -1
    for k, v in kw.items():
        p[P[k.upper()]] = int(v)
    return p


def decode_p(p, llr, out_bytes, pull=None, pull_stride=0, trace=None):
    """llr: int8 [n, num_llr], rows exactly num_llr apart; returns (rc, n_iter[n], out[n, out_bytes])"""
    n = int(p[names("P")["N_BLOCKS"]])
    assert llr.dtype == np.int8 and llr.flags.c_contiguous and llr.shape[0] == n
    out = np.full((n, out_bytes), OUT_INIT, np.uint8)
    n_iter = np.full(n, -7, np.int32)
    rc = lib().dec_emul_decode(p.ctypes.data, llr.ctypes.data, llr.shape[1], out.ctypes.data, out_bytes, n_iter.ctypes.data,
                               None if pull is None else pull.ctypes.data, pull_stride, None if trace is None else trace.ctypes.data)
    return rc, n_iter, out


if __name__ == "__main__":
    z = np.load(sys.argv[1])
    rc, n_iter, out = decode_p(z["p"], np.ascontiguousarray(z["llr"]), int(z["out_bytes"]))
    P = names("P")
    p = z["p"]
    takes = lib().dec_emul_takes_zc_kernel(int(p[P["BG"]]), int(p[P["Z"]]), int(p[P["R"]]), int(p[P["SHAPE"]]))
    np.savez(sys.argv[2], rc=rc, n_iter=n_iter, out=out, takes_zc=takes)
