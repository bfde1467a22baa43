"""The fast decoder's schedule knobs (ldpc_graph.c: NRLDPC_HIP_FAST_WAVES, _EXT_GLOBAL, _BN_SHORT, _BN_GROUP, _CN_DOUBLE, _PAIR19):
the values the tests turn them to, the codes they are tried on, and -- from the descriptors the table builder writes under each
value -- the codes on which a value changes anything.  Shared by tests/test_switches_host.py (emulator, no GPU) and
tests/test_gpu_switches.py (the same values on the device): the GPU half runs a value on the codes this module found affected.

ldpc_graph.c reads the knobs at every descriptor build and the emulator caches nothing, so a value is set in os.environ around the
calls that build descriptors and taken out again (knob_env)."""
import contextlib
import ctypes as C
import functools
import os
from pathlib import Path

PREFIX = "NRLDPC_HIP_"
KNOBS = ("FAST_WAVES", "EXT_GLOBAL", "BN_SHORT", "BN_GROUP", "CN_DOUBLE", "PAIR19")
# label -> environment (names without the prefix)
KNOB_VALUES = {f"{k}={v}": {k: str(v)} for k, vals in (("FAST_WAVES", (1, 2, 3, 5, 7, 9, 13, 16)), ("EXT_GLOBAL", (0, 1)),
                                                        ("BN_SHORT", (0, 3, 30)), ("BN_GROUP", (1, 2, 5)),
                                                        ("CN_DOUBLE", (0, 3, 4)), ("PAIR19", (0,))) for v in vals}
KNOB_VALUES["combined"] = dict(FAST_WAVES="7", EXT_GLOBAL="1", BN_SHORT="3", BN_GROUP="2", CN_DOUBLE="3", PAIR19="0")
# (BG, Zc, decoder rate mode): BG1 384 at 1/3, 2/3, 8/9; BG1 352 at 2/3; BG1 64 at 1/3; BG2 384 at 1/5; BG2 208 at 1/3;
# BG2 64 at 2/3; BG2 16 at 1/5
CODES = ((1, 384, 13), (1, 384, 23), (1, 384, 89), (1, 352, 23), (1, 64, 13), (2, 384, 15), (2, 208, 13), (2, 64, 23), (2, 16, 15))
SHAPES = {"throughput": 0, "latency": 1}      # ldpc_graph.h LDPC_SHAPE_*
# (label, code, shape) for which the builder gives the fast section up (f_ok = 0): BN_SHORT=30 pads every column's list of BG1
# Zc = 384 R = 1/3 to the longest one, and with the extension LLRs staged in LDS -- which the latency shape always does -- the
# workgroup no longer fits 160 KiB.  The library then switches the fast section off for the code in BOTH shapes (ldpc_api.cpp
# get_code_impl) and the generic kernel serves every call: falls back, same results.
FALLS_BACK = {("BN_SHORT=30", (1, 384, 13), "latency")}
INFO_FIELDS = ("f_ok", "threads", "lds_bytes", "cn_tasks", "bn_tickets", "ext_global", "pair19", "wg_per_cu")


def full_env(short):
    return {PREFIX + k: v for k, v in short.items()}


@contextlib.contextmanager
def knob_env(short):
    """the six knobs set to `short` (absent ones unset) while the block runs; the process' own values afterwards"""
    saved = {PREFIX + k: os.environ.pop(PREFIX + k, None) for k in KNOBS}
    try:
        os.environ.update(full_env(short))
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def emul_lib():
    L = C.CDLL(str(Path(__file__).resolve().parent / "emul" / "libldpc_emul.so"))
    L.ldpc_emul_desc_shape.argtypes = [C.c_int] * 4 + [C.c_void_p]
    L.ldpc_emul_fast_info.argtypes = [C.c_int] * 4 + [C.c_void_p]
    for f in (L.ldpc_emul_decode, L.ldpc_emul_decode_fast):
        f.argtypes = [C.c_int] * 8 + [C.c_void_p, C.c_void_p]
    return L


def descriptor(BG, Z, R, shape):
    """the descriptor's bytes as the table builder writes them under the knobs set right now"""
    L = emul_lib()
    buf = C.create_string_buffer(L.ldpc_emul_desc_size())
    assert L.ldpc_emul_desc_shape(BG, Z, R, SHAPES[shape], buf) == 0
    return buf.raw


def fast_info(BG, Z, R, shape="throughput"):
    a = (C.c_int * 8)()
    assert emul_lib().ldpc_emul_fast_info(BG, Z, R, SHAPES[shape], a) == 0
    return dict(zip(INFO_FIELDS, a))


@functools.lru_cache(maxsize=None)
def affected_codes():
    """{label: ((BG, Zc, R, shape), ...)}: the codes of CODES and the workgroup shapes whose descriptor under the knob value
    differs from the default's in at least one byte.  Needs the emulator library (the `built` fixture)."""
    with knob_env({}):
        base = {(c, s): descriptor(*c, s) for c in CODES for s in SHAPES}
    out = {}
    for label, short in KNOB_VALUES.items():
        with knob_env(short):
            out[label] = tuple(c + (s,) for c in CODES for s in SHAPES if descriptor(*c, s) != base[(c, s)])
    return out


def affected_throughput_codes(labels):
    """the (BG, Zc, R) whose throughput-shape descriptor one of the values `labels` changes, in CODES order"""
    hit = {c[:3] for lab in labels for c in affected_codes()[lab] if c[3] == "throughput"}
    return [c for c in CODES if c in hit]


def __getattr__(name):
    """AFFECTED: affected_codes() as a module constant, computed at its first use (the emulator library is built by then)"""
    if name == "AFFECTED":
        return affected_codes()
    raise AttributeError(name)
