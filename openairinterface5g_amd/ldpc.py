"""Python host side of libldpc_hip.so -- mirrors the reference's LDPC plugin interface.

The reference exposes the codec as ``ldpc_interface_t {LDPCinit, LDPCshutdown, LDPCdecoder, LDPCencoder}``
(openair1/PHY/CODING/nrLDPC_extern.h:27-33) taking ``t_nrLDPC_dec_params`` / ``encoder_implemparams_t``
(nrLDPC_types.h:84-97, nrLDPC_defs.h:40-66).  This module binds the same four symbols plus the batched
entry points of include/nrLDPC_hip.h with ctypes; argument names and meaning follow the reference.

There is no fallback: if the shared library is missing or no GPU is usable, calls raise.
torch is used only as the owner of device memory and streams for the ``*_device`` calls.
"""
import ctypes as C
import os
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "lib" / "libldpc_hip.so"

# e_nrLDPC_outMode (nrLDPC_types.h:75-79)
nrLDPC_outMode_BIT, nrLDPC_outMode_BITINT8, nrLDPC_outMode_LLRINT8 = 0, 1, 2
# coding_defs.h:33-36
CRC24_A, CRC24_B, CRC16, CRC8 = 0, 1, 2, 3
MEM_HOST, MEM_DEVICE = 0, 1
MEM_HARQ_DEVICE, MEM_HARQ_LIBRARY = 2, 4   # OR-ed into mem for nrLDPC_hip_ulsch_decode: where the soft buffers live

NCOLS = {(1, 13): 68, (1, 23): 35, (1, 89): 27, (2, 15): 52, (2, 13): 32, (2, 23): 17}
LIFT_SIZES = sorted(a * (1 << j) for a in (2, 3, 5, 7, 9, 11, 13, 15) for j in range(8) if a * (1 << j) <= 384)

CHECK_CRC_T = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint8)


class t_nrLDPC_dec_params(C.Structure):
    """nrLDPC_types.h:84-97"""
    _fields_ = [("BG", C.c_uint8), ("Z", C.c_uint16), ("R", C.c_uint8), ("F", C.c_uint16), ("Qm", C.c_uint8),
                ("rv", C.c_uint8), ("numMaxIter", C.c_uint8), ("E", C.c_int), ("outMode", C.c_int),
                ("crc_type", C.c_int), ("check_crc", C.c_void_p), ("setCombIn", C.c_uint8)]


class encoder_implemparams_t(C.Structure):
    """nrLDPC_defs.h:40-66"""
    _fields_ = [("n_segments", C.c_uint), ("macro_num", C.c_uint), ("gen_code", C.c_ubyte),
                ("tinput", C.c_void_p), ("tprep", C.c_void_p), ("tparity", C.c_void_p), ("toutput", C.c_void_p),
                ("Kr", C.c_int), ("Kb", C.c_uint32), ("Zc", C.c_uint32), ("harq", C.c_void_p), ("BG", C.c_uint8),
                ("output", C.c_void_p), ("K", C.c_uint32), ("F", C.c_uint32), ("Qm", C.c_uint8), ("E", C.c_uint32),
                ("G", C.c_uint), ("rv", C.c_uint8)]


class time_stats_t(C.Structure):
    """common/utils/time_meas.h:61-74 (x86-64)"""
    _fields_ = [("in_", C.c_longlong), ("diff", C.c_longlong), ("p_time", C.c_longlong), ("diff_square", C.c_double),
                ("max", C.c_longlong), ("trials", C.c_int), ("meas_flag", C.c_int), ("meas_name", C.c_char_p),
                ("meas_index", C.c_int), ("meas_enabled", C.c_int), ("tpoolmsg", C.c_void_p), ("tstatptr", C.c_void_p)]


class t_nrLDPC_time_stats(C.Structure):
    """nrLDPC_types.h:115-127"""
    _fields_ = [(n, time_stats_t) for n in ("llr2llrProcBuf", "llr2CnProcBuf", "cnProc", "cnProcPc", "bnProcPc", "bnProc",
                                            "cn2bnProcBuf", "bn2cnProcBuf", "llrRes2llrOut", "llr2bit", "total")]


class decode_abort_t(C.Structure):
    """openair1/PHY/defs_common.h:998-1001 (pthread_mutex_t is 40 bytes on x86-64 glibc; all-zero = initialised)"""
    _fields_ = [("mutex_failure", C.c_uint64 * 5), ("failed", C.c_bool)]


class nrLDPC_hip_dec_batch_t(C.Structure):
    _fields_ = [("params", t_nrLDPC_dec_params), ("n_blocks", C.c_uint32), ("llr", C.c_void_p),
                ("llr_stride", C.c_uint32), ("out", C.c_void_p), ("out_stride", C.c_uint32), ("n_iter", C.c_void_p),
                ("mem", C.c_int32), ("stream", C.c_void_p), ("kernel", C.c_int32)]


class nrLDPC_hip_dec_job_t(C.Structure):
    _fields_ = [("params", t_nrLDPC_dec_params), ("llr", C.c_void_p), ("out", C.c_void_p)]


class nrLDPC_hip_enc_batch_t(C.Structure):
    _fields_ = [("BG", C.c_uint8), ("Zc", C.c_uint16), ("Kb", C.c_uint8), ("n_blocks", C.c_uint32),
                ("in_", C.c_void_p), ("in_stride", C.c_uint32), ("out", C.c_void_p), ("out_stride", C.c_uint32),
                ("mem", C.c_int32), ("stream", C.c_void_p)]


_user_predicates = []   # CFUNCTYPE objects of caller-supplied predicates must outlive the parameter blocks that hold them


def device_crc_pointer():
    """Address of the library's nrLDPC_hip_check_crc: in t_nrLDPC_dec_params.check_crc it selects the CRC stop that the GPU
    evaluates (as the host executable's own `check_crc` does); any other pointer is called on the host (nrLDPC_hip.h)."""
    return C.cast(load_library().nrLDPC_hip_check_crc, C.c_void_p).value

EXPORTS = ["LDPCinit", "LDPCshutdown", "LDPCdecoder", "LDPCencoder", "ldpc_checkbuildver", "ldpc_autoinit", "LDPCdecoder_batch", "LDPCencoder_batch",
           "LDPCdecoder_jobs", "nrLDPC_hip_checkbuildver", "nrLDPC_hip_check_crc",
           "nrLDPC_hip_num_llr", "nrLDPC_hip_out_bytes", "nrLDPC_hip_lds_bytes", "nrLDPC_hip_code_info", "nrLDPC_hip_last_error",
           "nrLDPC_hip_version", "nrLDPC_hip_server_stats"]

_lib = None


def load_library(path=None, mode=None):
    """dlopen libldpc_hip.so (the analogue of load_LDPClib, nrLDPC_load.c:45-75). Raises if it is missing.
    mode: dlopen flags of the first load (default RTLD_NOW | RTLD_GLOBAL; the reference's loader uses
    RTLD_LAZY | RTLD_NODELETE | RTLD_GLOBAL, load_module_shlib.c:160)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else Path(os.environ.get("NRLDPC_HIP_LIB", LIB_PATH))   # (env: A/B builds of the library)
    if not p.exists():
        raise RuntimeError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           f"or `make -C {_PKG / 'csrc'}` -- there is no CPU fallback")
    L = C.CDLL(str(p), mode=os.RTLD_NOW | os.RTLD_GLOBAL if mode is None else mode)
    L.LDPCinit.restype = C.c_int32
    L.LDPCshutdown.restype = C.c_int32
    L.LDPCdecoder.restype = C.c_int32
    L.LDPCdecoder.argtypes = [C.POINTER(t_nrLDPC_dec_params), C.c_uint8, C.c_uint8, C.c_uint8, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p]
    L.LDPCencoder.restype = C.c_int32
    L.LDPCencoder.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(encoder_implemparams_t)]
    L.LDPCdecoder_batch.restype = C.c_int32
    L.LDPCdecoder_batch.argtypes = [C.POINTER(nrLDPC_hip_dec_batch_t)]
    L.LDPCencoder_batch.restype = C.c_int32
    L.LDPCencoder_batch.argtypes = [C.POINTER(nrLDPC_hip_enc_batch_t)]
    for n in ("nrLDPC_hip_num_llr", "nrLDPC_hip_lds_bytes"):
        getattr(L, n).argtypes = [C.c_int] * 3
        getattr(L, n).restype = C.c_int32
    L.nrLDPC_hip_out_bytes.argtypes = [C.c_int] * 4
    L.nrLDPC_hip_out_bytes.restype = C.c_int32
    L.nrLDPC_hip_last_error.restype = C.c_char_p
    L.nrLDPC_hip_version.restype = C.c_char_p
    if path is None:
        _lib = L
    return L


def last_error():
    return load_library().nrLDPC_hip_last_error().decode()


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {last_error()}")


def LDPCinit():
    """nrLDPC_decoder.c:162.  Raises when no MI355X/HIP device is usable."""
    _check(load_library().LDPCinit(), "LDPCinit")
    return 0


def LDPCshutdown():
    return load_library().LDPCshutdown()


def server_stats():
    """State of the resident submission path behind LDPCdecoder / LDPCencoder (nrLDPC_hip_server_stats)."""
    L = load_library()
    a = (C.c_int64 * 8)()
    L.nrLDPC_hip_server_stats.argtypes = [C.POINTER(C.c_int64)]
    L.nrLDPC_hip_server_stats(a)
    return dict(status=int(a[0]), slots=int(a[1]), launches=int(a[2]), calls=int(a[3]), gpu_stage_ns=int(a[4]),
                gpu_decode_ns=int(a[5]), host_wait_ns=int(a[6]), host_call_ns=int(a[7]))


def num_llr(BG, Z, R):
    return NCOLS[(BG, R)] * Z


def code_info(BG, Z, R):
    """Shape of a code and of the decoder launch that serves it (nrLDPC_hip_code_info)."""
    L = load_library()
    a = (C.c_int32 * 8)()
    L.nrLDPC_hip_code_info.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]
    if L.nrLDPC_hip_code_info(BG, Z, R, a) != 0:
        raise ValueError("invalid code")
    return dict(nrows=a[0], ncols=a[1], nedges=a[2], kernel="fast" if a[3] else "generic", threads=a[4],
                lds_kib=round(a[5] / 1024, 1), cn_tasks=a[6], bn_tasks=a[7])


def out_bytes(BG, Z, R, outMode=nrLDPC_outMode_BIT):
    n = num_llr(BG, Z, R)
    return ((n + 31) // 32) * 4 if outMode == nrLDPC_outMode_BIT else n


def make_dec_params(BG, Z, R, numMaxIter=8, outMode=nrLDPC_outMode_BIT, check_crc=False, E=0, crc_type=CRC24_B):
    p = t_nrLDPC_dec_params(BG=BG, Z=Z, R=R, numMaxIter=numMaxIter, outMode=outMode, E=E, crc_type=crc_type)
    if callable(check_crc):      # a caller's own predicate (decoded_bytes_ptr, n, crc_type) -> int: called on the host
        cb = CHECK_CRC_T(check_crc)
        p._check_crc_keepalive = cb      # lives as long as the parameter block that points at it ...
        _user_predicates.append(cb)      # ... and a little longer for by-value copies of the block (job arrays)
        del _user_predicates[:-64]
        p.check_crc = C.cast(cb, C.c_void_p)
    elif check_crc:
        p.check_crc = device_crc_pointer()
    return p


def LDPCdecoder(p_decParams, p_llr, p_out=None, ab=None, harq_pid=0, ulsch_id=0, C_=0, profiler=None):
    """One code block through the reference's own entry point (nrLDPC_decoder.c:172).
    p_llr: int8[ncols*Z]; returns (numIter, p_out).  profiler: optional t_nrLDPC_time_stats."""
    L = load_library()
    p_llr = np.ascontiguousarray(p_llr, dtype=np.int8)
    nb = out_bytes(p_decParams.BG, p_decParams.Z, p_decParams.R, p_decParams.outMode)
    if p_out is None:
        p_out = np.zeros(nb, dtype=np.uint8)
    n = L.LDPCdecoder(C.byref(p_decParams), harq_pid, ulsch_id, C_, p_llr.ctypes.data, p_out.ctypes.data,
                      C.addressof(profiler) if profiler is not None else None,
                      C.addressof(ab) if ab is not None else None)
    if n < 0:
        raise RuntimeError(f"LDPCdecoder failed: {last_error()}")
    return n, p_out


def raw_decoder_call(p_decParams):
    """(call, keep): `call(llr_address, out_address) -> numIter` is the bare C entry point LDPCdecoder with everything but
    the two buffer addresses bound beforehand -- for callers that time the call itself, as ldpctest does with
    start_meas / stop_meas around `LDPCdecoder(...)` (ldpctest.c:329-334), without this module's per-call marshalling."""
    L = load_library()
    proto = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_uint8, C.c_uint8, C.c_uint8, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
    fn = proto(("LDPCdecoder", L))   # its own prototype object: L.LDPCdecoder keeps the typed one
    pref = C.cast(C.pointer(p_decParams), C.c_void_p)

    def call(llr_address, out_address):
        return fn(pref, 0, 0, 0, llr_address, out_address, None, None)
    return call, (p_decParams, pref)


def LDPCencoder(inputs, BG, Zc, Kb=None, n_segments=None, macro_num=0, meters=None, block_length=None):
    """Up to 8 segments through the reference entry point (ldpc_encoder_optim8segmulti.c:46).
    inputs: list of uint8[K/8]; returns list of uint8[(66|50)*Zc] (one bit per byte) for ALL n_segments
    (entries outside this macro group are left zero).  block_length: ldpctest's -l when it is shorter than K = 22|10 * Zc
    (impp->K; the code word is then cut to 3|5 * block_length bytes, ldpc_encoder.c:82-92,248-251)."""
    L = load_library()
    kbf = 22 if BG == 1 else 10
    K = kbf * Zc if block_length is None else block_length
    n_segments = len(inputs) if n_segments is None else n_segments
    ins = [np.ascontiguousarray(np.concatenate([np.asarray(i, dtype=np.uint8), np.zeros(8, np.uint8)])) for i in inputs]
    outs = [np.zeros(68 * 384, dtype=np.uint8) for _ in range(n_segments)]
    ip = (C.c_void_p * n_segments)(*[a.ctypes.data for a in ins])
    op = (C.c_void_p * n_segments)(*[a.ctypes.data for a in outs])
    impp = encoder_implemparams_t(n_segments=n_segments, macro_num=macro_num, gen_code=0, Kr=K,
                                  Kb=kbf if Kb is None else Kb, Zc=Zc, BG=BG, K=K, E=K)
    if meters is not None:      # four time_stats_t: tinput, tprep, tparity, toutput (nrLDPC_defs.h:44-47)
        impp.tinput, impp.tprep, impp.tparity, impp.toutput = (C.addressof(m) for m in meters)
    rc = L.LDPCencoder(ip, op, C.byref(impp))
    _check(rc, "LDPCencoder")
    if rc != 0:     # the default reference library's value (ldpc_encoder_optim8segmulti.c:213), not ldpc_encoder.c:251's length
        raise RuntimeError(f"LDPCencoder returned {rc}, expected 0")
    N = (66 if BG == 1 else 50) * Zc if block_length is None else (3 if BG == 1 else 5) * block_length
    return [o[:N] for o in outs]


# ---- the reference's offload plugin slot (ldpc_interface_offload, "_t2"): libldpc_hip_t2.so ------------------------------
EXPORTS += ["nrLDPC_hip_offload_init", "nrLDPC_hip_offload_decoder", "nrLDPC_hip_offload_encoder"]
T2_EXPORTS = ["LDPCinit", "LDPCshutdown", "LDPCdecoder", "LDPCencoder", "ldpc_checkbuildver"]
_t2 = None


def load_offload_library(mode=None, alone=False):
    """dlopen libldpc_hip_t2.so the way load_LDPClib("_t2", &ldpc_interface_offload) does (nr_init.c:138-139,
    nrLDPC_load.c:45-75) and run its LDPCinit.  Raises if the library is missing or no GPU is usable.
    mode: dlopen flags of the first load (default: ctypes' own); alone: do not load libldpc_hip.so first -- it then comes
    in through the offload library's DT_NEEDED entry and $ORIGIN, as in a process that uses the offload slot only."""
    global _t2
    if _t2 is None:
        if not alone:
            load_library()
        path = Path(os.environ.get("NRLDPC_HIP_T2_LIB", Path(LIB_PATH).parent / "libldpc_hip_t2.so"))
        if not path.exists():
            raise RuntimeError(f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)")
        L = C.CDLL(str(path)) if mode is None else C.CDLL(str(path), mode=mode)
        for name in T2_EXPORTS:
            getattr(L, name)
        L.LDPCdecoder.restype = C.c_int32
        L.LDPCdecoder.argtypes = [C.c_void_p, C.c_uint8, C.c_uint8, C.c_uint8, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.LDPCencoder.restype = C.c_int32
        L.LDPCencoder.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        if L.LDPCinit() != 0:
            raise RuntimeError(f"offload LDPCinit failed: {last_error()}")
        _t2 = L
    return _t2


def offload_decoder(BG, Z, R, llr, Qm, rv, F, setCombIn, ulsch_id=0, r=0, harq_pid=0, numMaxIter=8):
    """One segment through the offload slot's LDPCdecoder (nrLDPC_decoder_offload.c:1036, caller nr_ulsch_decoding.c:225-268):
    llr = the E received soft values as int8 in transmission order.  Returns (passes, decoded bytes uint8[ceil(K/8)])."""
    L = load_offload_library()
    llr = np.ascontiguousarray(llr, dtype=np.int8)
    p = t_nrLDPC_dec_params(BG=BG, Z=Z, R=R, F=F, Qm=Qm, rv=rv, numMaxIter=numMaxIter, E=llr.size, setCombIn=1 if setCombIn else 0)
    K = (22 if BG == 1 else 10) * Z
    out = np.zeros((K + 7) // 8 + 64, dtype=np.uint8)
    n = L.LDPCdecoder(C.addressof(p), harq_pid, ulsch_id, r, llr.ctypes.data, out.ctypes.data, None, None)
    if n < 0:
        raise RuntimeError(f"offload LDPCdecoder failed: {last_error()}")
    assert not out[(K + 7) // 8:].any()
    return n, out[:(K + 7) // 8]


def offload_encoder(BG, Zc, segment, F, E, Qm, rv, Kb=None):
    """One segment through the offload slot's LDPCencoder (nrLDPC_decoder_offload.c:1094, caller nr_dlsch_coding.c:366-383):
    segment = its K - F bits (uint8, MSB first).  Returns the E rate-matched, interleaved bits, one per byte."""
    L = load_offload_library()
    K = (22 if BG == 1 else 10) * Zc
    seg = np.ascontiguousarray(np.asarray(segment, dtype=np.uint8)[:(K - F) // 8])
    out = np.full(E + 64, 0xEE, dtype=np.uint8)
    ip = (C.c_void_p * 1)(seg.ctypes.data)
    op = (C.c_void_p * 1)(out.ctypes.data)
    impp = encoder_implemparams_t(n_segments=1, macro_num=0, Kr=K, Kb=(22 if BG == 1 else 10) if Kb is None else Kb, Zc=Zc, BG=BG,
                                  K=K, F=F, Qm=Qm, E=E, rv=rv)
    rc = L.LDPCencoder(C.addressof(ip), C.addressof(op), C.addressof(impp))
    if rc != 0:
        raise RuntimeError(f"offload LDPCencoder failed: {last_error()}")
    assert (out[E:] == 0xEE).all()
    return out[:E]


def decode_batch_host(BG, Z, R, llr, numMaxIter=8, outMode=nrLDPC_outMode_BIT, check_crc=False, E=0,
                      crc_type=CRC24_B, out=None, kernel=0):
    """llr: int8[n_blocks, >= ncols*Z] host array. Returns (n_iter int32[n], out uint8[n, out_bytes])."""
    L = load_library()
    llr = np.ascontiguousarray(llr, dtype=np.int8)
    n = llr.shape[0]
    ob = out_bytes(BG, Z, R, outMode)
    stride = (ob + 3) // 4 * 4
    if out is None:
        out = np.zeros((n, stride), dtype=np.uint8)
    it = np.zeros(n, dtype=np.int32)
    assert llr.ndim == 2 and out.ndim == 2 and out.flags.c_contiguous and out.shape[0] == n
    # (strides of a length-1 axis are arbitrary in numpy, so derive the row pitch from the shape)
    b = nrLDPC_hip_dec_batch_t(params=make_dec_params(BG, Z, R, numMaxIter, outMode, check_crc, E, crc_type),
                               n_blocks=n, llr=llr.ctypes.data, llr_stride=llr.shape[1], out=out.ctypes.data,
                               out_stride=out.shape[1], n_iter=it.ctypes.data, mem=MEM_HOST, stream=None, kernel=kernel)
    _check(L.LDPCdecoder_batch(C.byref(b)), "LDPCdecoder_batch")
    return it, out[:, :ob]


def decode_batch_device(BG, Z, R, llr, out, n_iter, numMaxIter=8, outMode=nrLDPC_outMode_BIT, check_crc=False, E=0,
                        crc_type=CRC24_B, stream=None, kernel=0):
    """Enqueue a decode of device-resident blocks (torch tensors: llr int8[n, stride], out uint8[n, stride'],
    n_iter int32[n]) on `stream` (default: torch's current stream). Asynchronous."""
    import torch
    L = load_library()
    assert llr.is_cuda and out.is_cuda and n_iter.is_cuda and llr.dtype == torch.int8 and n_iter.dtype == torch.int32
    assert llr.stride(1) == 1 and out.stride(1) == 1 and n_iter.is_contiguous()
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    b = nrLDPC_hip_dec_batch_t(params=make_dec_params(BG, Z, R, numMaxIter, outMode, check_crc, E, crc_type),
                               n_blocks=llr.shape[0], llr=llr.data_ptr(), llr_stride=llr.stride(0) * llr.element_size(),
                               out=out.data_ptr(), out_stride=out.stride(0) * out.element_size(),
                               n_iter=n_iter.data_ptr(), mem=MEM_DEVICE, stream=s, kernel=kernel)
    _check(L.LDPCdecoder_batch(C.byref(b)), "LDPCdecoder_batch")


class PreparedDecJobs:
    """A MIXED batch of code blocks (LDPCdecoder_jobs): blocks = list of dict(BG, Z, R, llr=torch int8 row on the GPU,
    out=torch uint8 row, numMaxIter=8, E=0, crc_type=CRC24_B); all with one outMode / stop mode.  Marshalled once,
    submitted many times; decode() only enqueues on the stream.  n_iter: torch int32 [len(blocks)]."""

    def __init__(self, blocks, n_iter, outMode=nrLDPC_outMode_BIT, check_crc=False, stream=None):
        import torch
        self._lib = load_library()
        self._lib.LDPCdecoder_jobs.argtypes = [C.POINTER(nrLDPC_hip_dec_job_t), C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p]
        self._lib.LDPCdecoder_jobs.restype = C.c_int32
        self._keep = (blocks, n_iter)
        self.arr = (nrLDPC_hip_dec_job_t * len(blocks))()
        for i, b in enumerate(blocks):
            assert b["llr"].is_cuda and b["out"].is_cuda and b["llr"].is_contiguous() and b["out"].is_contiguous()
            self.arr[i].params = make_dec_params(b["BG"], b["Z"], b["R"], b.get("numMaxIter", 8), outMode, check_crc, b.get("E", 0),
                                                 b.get("crc_type", CRC24_B))
            self.arr[i].llr = b["llr"].data_ptr()
            self.arr[i].out = b["out"].data_ptr()
        assert n_iter.is_cuda and n_iter.dtype == torch.int32 and n_iter.numel() >= len(blocks)
        self.n, self.n_iter = len(blocks), n_iter
        self.stream = torch.cuda.current_stream().cuda_stream if stream is None else stream

    def decode(self):
        _check(self._lib.LDPCdecoder_jobs(self.arr, self.n, self.n_iter.data_ptr(), MEM_DEVICE, self.stream), "LDPCdecoder_jobs")


def encode_batch_host(BG, Zc, info, Kb=None):
    """info: uint8[n_blocks, >= K/8] host array (MSB first). Returns uint8[n_blocks, (66|50)*Zc], one bit per byte."""
    L = load_library()
    info = np.ascontiguousarray(info, dtype=np.uint8)
    assert info.ndim == 2
    n = info.shape[0]
    N = (66 if BG == 1 else 50) * Zc
    out = np.zeros((n, N), dtype=np.uint8)
    b = nrLDPC_hip_enc_batch_t(BG=BG, Zc=Zc, Kb=(22 if BG == 1 else 10) if Kb is None else Kb, n_blocks=n,
                               in_=info.ctypes.data, in_stride=info.shape[1], out=out.ctypes.data,
                               out_stride=out.shape[1], mem=MEM_HOST, stream=None)
    _check(L.LDPCencoder_batch(C.byref(b)), "LDPCencoder_batch")
    return out


def encode_batch_device(BG, Zc, info, out, Kb=None, stream=None):
    """info: torch uint8[n, >= K/8], out: torch uint8[n, >= (66|50)*Zc], both on the GPU. Asynchronous."""
    import torch
    L = load_library()
    assert info.is_cuda and out.is_cuda and info.stride(1) == 1 and out.stride(1) == 1
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    b = nrLDPC_hip_enc_batch_t(BG=BG, Zc=Zc, Kb=(22 if BG == 1 else 10) if Kb is None else Kb, n_blocks=info.shape[0],
                               in_=info.data_ptr(), in_stride=info.stride(0), out=out.data_ptr(),
                               out_stride=out.stride(0), mem=MEM_DEVICE, stream=s)
    _check(L.LDPCencoder_batch(C.byref(b)), "LDPCencoder_batch")


# ---------------------------------------------------------------------------------------------------------
# Transport-block chain (include/nrLDPC_hip.h: nrLDPC_hip_dlsch_encode / nrLDPC_hip_ulsch_decode)
# ---------------------------------------------------------------------------------------------------------
class nrLDPC_hip_tb_t(C.Structure):
    _fields_ = [("A", C.c_uint32), ("G", C.c_uint32), ("tbslbrm", C.c_uint32), ("BG", C.c_uint8), ("Qm", C.c_uint8),
                ("Nl", C.c_uint8), ("rv", C.c_uint8), ("numMaxIter", C.c_uint8), ("round", C.c_uint8),
                ("llrLen", C.c_int32), ("payload_off", C.c_uint64), ("coded_off", C.c_uint64), ("harq_off", C.c_uint64)]


class nrLDPC_hip_tb_batch_t(C.Structure):
    _fields_ = [("n_tb", C.c_uint32), ("tb", C.POINTER(nrLDPC_hip_tb_t)), ("payload", C.c_void_p), ("coded", C.c_void_p),
                ("harq", C.c_void_p), ("harq_stride", C.c_uint32), ("ack", C.c_void_p), ("iter_max", C.c_void_p),
                ("mem", C.c_int32), ("stream", C.c_void_p)]


class nrLDPC_hip_tb_scr_t(C.Structure):
    _fields_ = [("n_RNTI", C.c_uint32), ("Nid", C.c_uint16), ("q", C.c_uint8), ("pad", C.c_uint8)]


def _scr_array(scrambling, n):
    """(n_rnti, q, n_id) per transport block -> nrLDPC_hip_tb_scr_t[n] (the library checks the ranges)"""
    assert len(scrambling) == n
    arr = (nrLDPC_hip_tb_scr_t * n)()
    for i, (n_rnti, q, n_id) in enumerate(scrambling):
        arr[i] = nrLDPC_hip_tb_scr_t(n_RNTI=int(n_rnti) & 0xffffffff, Nid=int(n_id) & 0xffff, q=int(q) & 0xff, pad=0)
    return arr


EXPORTS += ["nrLDPC_hip_dlsch_encode_scrambled", "nrLDPC_hip_ulsch_decode_scrambled"]
EXPORTS += ["nrLDPC_hip_dlsch_encode", "nrLDPC_hip_ulsch_decode", "nrLDPC_hip_segmentation", "nrLDPC_hip_get_E",
            "nrLDPC_hip_get_R_ldpc_decoder", "nrLDPC_hip_harq_release", "nrLDPC_hip_harq_release_all", "nrLDPC_hip_harq_read",
            "nrLDPC_hip_host_alloc", "nrLDPC_hip_host_free", "nrLDPC_hip_host_register", "nrLDPC_hip_host_unregister",
            "nrLDPC_hip_chain_timing", "nrLDPC_hip_ulsch_decoder_columns"]
HARQ_STRIDE = 66 * 384


def _tb_lib():
    L = load_library()
    L.nrLDPC_hip_dlsch_encode.argtypes = [C.POINTER(nrLDPC_hip_tb_batch_t)]
    L.nrLDPC_hip_ulsch_decode.argtypes = [C.POINTER(nrLDPC_hip_tb_batch_t)]
    if hasattr(L, "nrLDPC_hip_dlsch_encode_scrambled"):
        L.nrLDPC_hip_dlsch_encode_scrambled.argtypes = [C.POINTER(nrLDPC_hip_tb_batch_t), C.POINTER(nrLDPC_hip_tb_scr_t)]
        L.nrLDPC_hip_ulsch_decode_scrambled.argtypes = [C.POINTER(nrLDPC_hip_tb_batch_t), C.POINTER(nrLDPC_hip_tb_scr_t)]
    if hasattr(L, "nrLDPC_hip_ulsch_decode_symbols"):
        L.nrLDPC_hip_ulsch_decode_symbols.argtypes = [C.POINTER(nrLDPC_hip_tb_batch_t), C.POINTER(nrLDPC_hip_tb_scr_t)]
    if hasattr(L, "nrLDPC_hip_dlsch_encode_symbols"):
        L.nrLDPC_hip_dlsch_encode_symbols.argtypes = [C.POINTER(nrLDPC_hip_tb_batch_t), C.POINTER(nrLDPC_hip_tb_scr_t)]
    L.nrLDPC_hip_segmentation.argtypes = [C.c_uint32, C.c_uint8] + [C.POINTER(C.c_uint32)] * 4
    L.nrLDPC_hip_segmentation.restype = C.c_int32
    L.nrLDPC_hip_get_E.argtypes = [C.c_uint32] * 5
    L.nrLDPC_hip_get_E.restype = C.c_uint32
    L.nrLDPC_hip_get_R_ldpc_decoder.argtypes = [C.c_int32] * 4 + [C.POINTER(C.c_int32), C.c_int32]
    L.nrLDPC_hip_get_R_ldpc_decoder.restype = C.c_int32
    if hasattr(L, "nrLDPC_hip_ulsch_decoder_columns"):
        L.nrLDPC_hip_ulsch_decoder_columns.argtypes = [C.c_int32] + [C.c_uint32] * 5 + [C.c_int32, C.c_uint32, C.c_int32, C.c_int32]
        L.nrLDPC_hip_ulsch_decoder_columns.restype = C.c_int32
    if hasattr(L, "nrLDPC_hip_harq_release"):       # (absent from older builds of the library loaded through NRLDPC_HIP_LIB for A/B runs)
        L.nrLDPC_hip_harq_release.argtypes = [C.c_uint64]
        L.nrLDPC_hip_harq_read.argtypes = [C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64]
        L.nrLDPC_hip_host_alloc.argtypes = [C.c_uint64]
        L.nrLDPC_hip_host_alloc.restype = C.c_void_p
        L.nrLDPC_hip_host_free.argtypes = [C.c_void_p]
        L.nrLDPC_hip_host_free.restype = None
        L.nrLDPC_hip_host_register.argtypes = [C.c_void_p, C.c_uint64]
        L.nrLDPC_hip_host_unregister.argtypes = [C.c_void_p]
        L.nrLDPC_hip_chain_timing.argtypes = [C.c_int32, C.c_void_p]
    return L


class PinnedArray:
    """A numpy array in page-locked host memory from nrLDPC_hip_host_alloc (what a C caller without the HIP runtime
    uses): the GPU reads it in place.  Keep the object alive while `a` is in use."""

    def __init__(self, shape, dtype):
        self._lib = _tb_lib()
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._p = self._lib.nrLDPC_hip_host_alloc(max(n, 1))
        if not self._p:
            raise RuntimeError("nrLDPC_hip_host_alloc failed: " + self._lib.nrLDPC_hip_last_error().decode())
        buf = (C.c_uint8 * max(n, 1)).from_address(self._p)
        self.a = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def __del__(self):
        if getattr(self, "_p", None):
            self._lib.nrLDPC_hip_host_free(self._p)
            self._p = None


def chain_timing(enable=True, read=False):
    """nrLDPC_hip_chain_timing: switch the per-stage HIP events of this thread's UL-SCH calls on / off; read=True returns
    the last recorded call's (de-matching, decoder / fused kernel, reassembly + verdict, sum) in microseconds."""
    L = _tb_lib()
    out = (C.c_float * 4)()
    _check(L.nrLDPC_hip_chain_timing(int(bool(enable)), out if read else None), "nrLDPC_hip_chain_timing")
    return tuple(out) if read else None


def harq_read(harq_id, n, first=0):
    """int16[n] of the soft buffers the library keeps for block `harq_id` (MEM_HARQ_LIBRARY); after a device-memory call:
    synchronise its stream first."""
    out = np.zeros(n, np.int16)
    _check(_tb_lib().nrLDPC_hip_harq_read(harq_id, out.ctypes.data, first, n), "nrLDPC_hip_harq_read")
    return out


def harq_release(harq_id=None):
    L = _tb_lib()
    return L.nrLDPC_hip_harq_release_all() if harq_id is None else L.nrLDPC_hip_harq_release(harq_id)


def nr_segmentation(B, BG):
    """Parameter part of nr_segmentation (nr_segmentation.c:32-140): dict(C, K, Z, F, Kb) or None."""
    L = _tb_lib()
    Cn, K, Z, F = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    kb = L.nrLDPC_hip_segmentation(B, BG, C.byref(Cn), C.byref(K), C.byref(Z), C.byref(F))
    return None if kb < 0 else dict(C=Cn.value, K=K.value, Z=Z.value, F=F.value, Kb=kb)


def nr_get_E(G, C_, Qm, Nl, r):
    return _tb_lib().nrLDPC_hip_get_E(G, C_, Qm, Nl, r)


def nr_get_R_ldpc_decoder(rv, E, BG, Z, llrLen, rnd):
    ll = C.c_int32(llrLen)
    R = _tb_lib().nrLDPC_hip_get_R_ldpc_decoder(rv, E, BG, Z, C.byref(ll), rnd)
    return R, ll.value


def ulsch_decoder_columns(BG, Zc, C_, F, K, tbslbrm, rv, E, rnd, R):
    """columns of the code graph nrLDPC_hip_ulsch_decode() runs a segment on (nrLDPC_hip.h)"""
    return _tb_lib().nrLDPC_hip_ulsch_decoder_columns(BG, Zc, C_, F, K, tbslbrm, rv, E, rnd, R)


def _tb_array(tbs, offs_payload, offs_coded, offs_harq, numMaxIter=8):
    arr = (nrLDPC_hip_tb_t * len(tbs))()
    for i, t in enumerate(tbs):
        arr[i] = nrLDPC_hip_tb_t(A=t["A"], G=t["G"], tbslbrm=t.get("tbslbrm", 0), BG=t["BG"], Qm=t["Qm"], Nl=t["Nl"],
                                 rv=t.get("rv", 0), numMaxIter=t.get("numMaxIter", numMaxIter), round=t.get("round", 0),
                                 llrLen=t.get("llrLen", 0), payload_off=offs_payload[i], coded_off=offs_coded[i],
                                 harq_off=offs_harq[i] if offs_harq is not None else 0)
    return arr


def dlsch_encode_host(tbs, payloads):
    """TX chain for a batch of transport blocks, host buffers.  tbs: list of dict(A, G, BG, Qm, Nl, rv, tbslbrm);
    payloads: list of uint8[A/8].  Returns list of uint8[G] (one bit per byte, the reference's `output`)."""
    L = _tb_lib()
    po = np.cumsum([0] + [(t["A"] // 8 + 15) // 16 * 16 for t in tbs])
    co = np.cumsum([0] + [(t["G"] + 15) // 16 * 16 for t in tbs])
    pay = np.zeros(int(po[-1]) + 16, np.uint8)
    for i, p in enumerate(payloads):
        pay[po[i]:po[i] + tbs[i]["A"] // 8] = np.asarray(p, np.uint8)[:tbs[i]["A"] // 8]
    coded = np.zeros(int(co[-1]) + 16, np.uint8)
    arr = _tb_array(tbs, po, co, None)
    b = nrLDPC_hip_tb_batch_t(n_tb=len(tbs), tb=arr, payload=pay.ctypes.data, coded=coded.ctypes.data, harq=None,
                              harq_stride=0, ack=None, iter_max=None, mem=MEM_HOST, stream=None)
    _check(L.nrLDPC_hip_dlsch_encode(C.byref(b)), "nrLDPC_hip_dlsch_encode")
    return [coded[co[i]:co[i] + tbs[i]["G"]].copy() for i in range(len(tbs))]


def ulsch_decode_host(tbs, llrs, harq, numMaxIter=8, harq_off=None, harq_ids=None, pinned=False, payload_off=None):
    """RX chain for a batch of transport blocks, host buffers.  llrs: list of int16[G]; harq: int16 array
    [total segments, HARQ_STRIDE] holding the soft buffers of all TBs back to back (updated in place); each tb dict
    may carry 'round' and 'llrLen' ('llrLen' is updated).  harq_off: explicit int16 offsets of the TBs' soft buffers in
    `harq` (any order, gaps allowed) instead of back to back.  Returns (payloads, ack bool[n], iter_max int32[n]).
    Soft buffers on the GPU while everything else stays on the host (what nr_ulsch_decoding's caller needs: the LLRs of a
    slot arrive in host memory, d[r] persists per HARQ process): `harq` a torch int16 CUDA tensor (MEM_HARQ_DEVICE), or
    harq=None with harq_ids = one id per TB (MEM_HARQ_LIBRARY: the library keeps them; harq_read() looks at them).
    pinned: the LLR array goes into page-locked memory (nrLDPC_hip_host_alloc) and is pulled by the GPU in place.
    payload_off: explicit byte offsets of the TBs' payloads in the call's payload array (any order) instead of back to back."""
    return _ulsch_decode_host(tbs, llrs, harq, numMaxIter, harq_off, harq_ids, pinned, payload_off, None)


def ulsch_decode_scrambled_host(tbs, llrs, harq, scrambling, numMaxIter=8, harq_off=None, harq_ids=None, pinned=False,
                                payload_off=None):
    """ulsch_decode_host on scrambled LLRs (nrLDPC_hip_ulsch_decode_scrambled): scrambling = one (n_rnti, q, n_id) per TB.
    The same results as codeword_unscrambling() of every TB's LLRs followed by ulsch_decode_host; `llrs` are only read."""
    return _ulsch_decode_host(tbs, llrs, harq, numMaxIter, harq_off, harq_ids, pinned, payload_off, _scr_array(scrambling, len(tbs)))


def ulsch_decode_symbols_host(tbs, records, harq, scrambling, numMaxIter=8, harq_off=None, harq_ids=None, pinned=False,
                              payload_off=None):
    """ulsch_decode_scrambled_host from symbol records (nrLDPC_hip_ulsch_decode_symbols): records[i] = TB i's int16[G] planar
    record (pack_symbol_records).  The same results as ulsch_llr() of every TB's symbols followed by
    ulsch_decode_scrambled_host."""
    return _ulsch_decode_host(tbs, records, harq, numMaxIter, harq_off, harq_ids, pinned, payload_off, _scr_array(scrambling, len(tbs)),
                              sym=True)


def _decode_call(L, b, scr, sym=False):
    if sym:
        _check(L.nrLDPC_hip_ulsch_decode_symbols(C.byref(b), scr), "nrLDPC_hip_ulsch_decode_symbols")
    elif scr is None:
        _check(L.nrLDPC_hip_ulsch_decode(C.byref(b)), "nrLDPC_hip_ulsch_decode")
    else:
        _check(L.nrLDPC_hip_ulsch_decode_scrambled(C.byref(b), scr), "nrLDPC_hip_ulsch_decode_scrambled")


def _ulsch_decode_host(tbs, llrs, harq, numMaxIter, harq_off, harq_ids, pinned, payload_off, scr, sym=False):
    L = _tb_lib()
    n = len(tbs)
    if harq_ids is not None or not isinstance(harq, np.ndarray):
        return _ulsch_decode_host_resident(L, tbs, llrs, harq, numMaxIter, harq_off, harq_ids, pinned, payload_off, scr, sym)
    po = np.cumsum([0] + [(t["A"] // 8 + 15) // 16 * 16 for t in tbs])
    pay_total = int(po[-1])
    if payload_off is not None:
        po = list(payload_off)
    co = np.cumsum([0] + [(t["G"] + 7) // 8 * 8 for t in tbs])
    segs = [nr_segmentation(t["A"] + (24 if t["A"] > 3824 else 16), t["BG"])["C"] for t in tbs]
    ho = np.cumsum([0] + [c * HARQ_STRIDE for c in segs])
    if harq_off is not None:
        ho = list(harq_off)
        assert len(ho) == n and all(o + c * HARQ_STRIDE <= harq.size for o, c in zip(ho, segs))
    assert harq.dtype == np.int16 and harq.flags.c_contiguous and harq.size >= max(o + c * HARQ_STRIDE for o, c in zip(ho, segs))
    pay = np.zeros(pay_total + 16, np.uint8)
    keep = PinnedArray(int(co[-1]) + 16, np.int16) if pinned else None
    llr = keep.a if pinned else np.zeros(int(co[-1]) + 16, np.int16)
    llr[:] = 0
    for i, x in enumerate(llrs):
        llr[co[i]:co[i] + tbs[i]["G"]] = x
    ack = np.zeros(n, np.uint8)
    itm = np.zeros(n, np.int32)
    arr = _tb_array(tbs, po, co, ho, numMaxIter)
    b = nrLDPC_hip_tb_batch_t(n_tb=n, tb=arr, payload=pay.ctypes.data, coded=llr.ctypes.data, harq=harq.ctypes.data,
                              harq_stride=HARQ_STRIDE, ack=ack.ctypes.data, iter_max=itm.ctypes.data, mem=MEM_HOST,
                              stream=None)
    _decode_call(L, b, scr, sym)
    for i, t in enumerate(tbs):
        t["llrLen"] = arr[i].llrLen
    return [pay[po[i]:po[i] + tbs[i]["A"] // 8].copy() for i in range(n)], ack.astype(bool), itm


def _ulsch_decode_host_resident(L, tbs, llrs, harq, numMaxIter, harq_off, harq_ids, pinned, payload_off=None, scr=None, sym=False):
    """host payload / LLRs / verdicts with the soft buffers resident on the GPU (see ulsch_decode_host)"""
    n = len(tbs)
    po = np.cumsum([0] + [(t["A"] // 8 + 15) // 16 * 16 for t in tbs])
    pay_total = int(po[-1])
    if payload_off is not None:
        po = list(payload_off)
    co = np.cumsum([0] + [(t["G"] + 7) // 8 * 8 for t in tbs])
    segs = [nr_segmentation(t["A"] + (24 if t["A"] > 3824 else 16), t["BG"])["C"] for t in tbs]
    if harq_ids is not None:
        assert harq is None and len(harq_ids) == n
        ho, hp, mem = list(harq_ids), None, MEM_HOST | MEM_HARQ_LIBRARY
    else:
        ho = list(harq_off) if harq_off is not None else list(np.cumsum([0] + [c * HARQ_STRIDE for c in segs])[:n])
        assert harq.is_cuda and harq.is_contiguous() and harq.numel() >= max(o + c * HARQ_STRIDE for o, c in zip(ho, segs))
        hp, mem = harq.data_ptr(), MEM_HOST | MEM_HARQ_DEVICE
    pay = np.zeros(pay_total + 16, np.uint8)
    keep = PinnedArray(int(co[-1]) + 16, np.int16) if pinned else None
    llr = keep.a if pinned else np.zeros(int(co[-1]) + 16, np.int16)
    llr[:] = 0
    for i, x in enumerate(llrs):
        llr[co[i]:co[i] + tbs[i]["G"]] = x
    ack = np.zeros(n, np.uint8)
    itm = np.zeros(n, np.int32)
    arr = _tb_array(tbs, po, co, ho, numMaxIter)
    b = nrLDPC_hip_tb_batch_t(n_tb=n, tb=arr, payload=pay.ctypes.data, coded=llr.ctypes.data, harq=hp,
                              harq_stride=HARQ_STRIDE, ack=ack.ctypes.data, iter_max=itm.ctypes.data, mem=mem, stream=None)
    _decode_call(L, b, scr, sym)
    for i, t in enumerate(tbs):
        t["llrLen"] = arr[i].llrLen
    return [pay[po[i]:po[i] + tbs[i]["A"] // 8].copy() for i in range(n)], ack.astype(bool), itm


def tb_layout(tbs):
    """Offsets used by the *_device transport-block calls: payload bytes, coded elements, harq int16 elements."""
    po = np.cumsum([0] + [(t["A"] // 8 + 15) // 16 * 16 for t in tbs])
    co = np.cumsum([0] + [(t["G"] + 15) // 16 * 16 for t in tbs])
    segs = [nr_segmentation(t["A"] + (24 if t["A"] > 3824 else 16), t["BG"])["C"] for t in tbs]
    ho = np.cumsum([0] + [c * HARQ_STRIDE for c in segs])
    return po, co, ho, segs


def tb_layout_packed(tbs):
    """Byte offsets of the TBs' packed words for the *_scrambled encode calls (4-byte aligned, ceil(G/32) words each, 16-byte
    spacing) and the bytes they span: (offsets, total)."""
    co = np.cumsum([0] + [((t["G"] + 31) // 32 * 4 + 15) // 16 * 16 for t in tbs])
    return co[:-1], int(co[-1])


def dlsch_encode_scrambled_host(tbs, payloads, scrambling):
    """dlsch_encode_host with scrambling (nrLDPC_hip_dlsch_encode_scrambled): scrambling = one (n_rnti, q, n_id) per TB.
    Returns a list of uint32[ceil(G/32)]: the words codeword_scrambling() makes of dlsch_encode_host's bits."""
    L = _tb_lib()
    po = np.cumsum([0] + [(t["A"] // 8 + 15) // 16 * 16 for t in tbs])
    co, total = tb_layout_packed(tbs)
    pay = np.zeros(int(po[-1]) + 16, np.uint8)
    for i, p in enumerate(payloads):
        pay[po[i]:po[i] + tbs[i]["A"] // 8] = np.asarray(p, np.uint8)[:tbs[i]["A"] // 8]
    coded = np.zeros(total // 4 + 4, np.uint32)
    arr = _tb_array(tbs, po, co, None)
    b = nrLDPC_hip_tb_batch_t(n_tb=len(tbs), tb=arr, payload=pay.ctypes.data, coded=coded.ctypes.data, harq=None,
                              harq_stride=0, ack=None, iter_max=None, mem=MEM_HOST, stream=None)
    _check(L.nrLDPC_hip_dlsch_encode_scrambled(C.byref(b), _scr_array(scrambling, len(tbs))), "nrLDPC_hip_dlsch_encode_scrambled")
    return [coded[co[i] // 4:co[i] // 4 + (tbs[i]["G"] + 31) // 32].copy() for i in range(len(tbs))]


def dlsch_encode_scrambled_device(tbs, payload, coded, scrambling, stream=None):
    """payload: torch uint8 [>= tb_layout po[-1]] on the GPU, coded: torch tensor on the GPU of >= tb_layout_packed total
    bytes (out: TB i's words at byte tb_layout_packed offset i).  Asynchronous."""
    import torch
    L = _tb_lib()
    po, _, _, _ = tb_layout(tbs)
    co, total = tb_layout_packed(tbs)
    assert payload.is_cuda and coded.is_cuda and payload.numel() >= po[-1] and coded.numel() * coded.element_size() >= total
    arr = _tb_array(tbs, po, co, None)
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    b = nrLDPC_hip_tb_batch_t(n_tb=len(tbs), tb=arr, payload=payload.data_ptr(), coded=coded.data_ptr(), harq=None,
                              harq_stride=0, ack=None, iter_max=None, mem=MEM_DEVICE, stream=s)
    _check(L.nrLDPC_hip_dlsch_encode_scrambled(C.byref(b), _scr_array(scrambling, len(tbs))), "nrLDPC_hip_dlsch_encode_scrambled")


def tb_layout_symbols(tbs):
    """Byte offsets of the TBs' layer-mapped points for nrLDPC_hip_dlsch_encode_symbols (4 G/Qm bytes each, 16-byte spacing)
    and the bytes they span: (offsets, total)."""
    co = np.cumsum([0] + [(4 * (t["G"] // t["Qm"]) + 15) // 16 * 16 for t in tbs])
    return co[:-1], int(co[-1])


def dlsch_encode_symbols_host(tbs, payloads, scrambling):
    """dlsch_encode_scrambled_host through modulation and layer mapping (nrLDPC_hip_dlsch_encode_symbols).  Returns a list of
    int16[Nl, G/(Qm Nl), 2]: TB i's layer planes, entry k of plane l = the point of codeword symbol k Nl + l."""
    L = _tb_lib()
    po = np.cumsum([0] + [(t["A"] // 8 + 15) // 16 * 16 for t in tbs])
    co, total = tb_layout_symbols(tbs)
    pay = np.zeros(int(po[-1]) + 16, np.uint8)
    for i, p in enumerate(payloads):
        pay[po[i]:po[i] + tbs[i]["A"] // 8] = np.asarray(p, np.uint8)[:tbs[i]["A"] // 8]
    coded = np.zeros(total // 2 + 8, np.int16)
    arr = _tb_array(tbs, po, co, None)
    b = nrLDPC_hip_tb_batch_t(n_tb=len(tbs), tb=arr, payload=pay.ctypes.data, coded=coded.ctypes.data, harq=None,
                              harq_stride=0, ack=None, iter_max=None, mem=MEM_HOST, stream=None)
    _check(L.nrLDPC_hip_dlsch_encode_symbols(C.byref(b), _scr_array(scrambling, len(tbs))), "nrLDPC_hip_dlsch_encode_symbols")
    out = []
    for i, t in enumerate(tbs):
        S = t["G"] // t["Qm"]
        out.append(coded[co[i] // 2:co[i] // 2 + 2 * S].reshape(t["Nl"], S // t["Nl"], 2).copy())
    return out


def dlsch_encode_symbols_device(tbs, payload, coded, scrambling, stream=None, coded_off=None):
    """payload: torch uint8 [>= tb_layout po[-1]] on the GPU, coded: torch tensor on the GPU of >= tb_layout_symbols total bytes
    (out: TB i's layer planes at byte tb_layout_symbols offset i, or at coded_off[i]).  Asynchronous."""
    import torch
    L = _tb_lib()
    po, _, _, _ = tb_layout(tbs)
    co, total = tb_layout_symbols(tbs)
    if coded_off is not None:
        co = list(coded_off)
        total = max(int(o) + 4 * (t["G"] // t["Qm"]) for o, t in zip(co, tbs))
    assert payload.is_cuda and coded.is_cuda and payload.numel() >= po[-1] and coded.numel() * coded.element_size() >= total
    arr = _tb_array(tbs, po, co, None)
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    b = nrLDPC_hip_tb_batch_t(n_tb=len(tbs), tb=arr, payload=payload.data_ptr(), coded=coded.data_ptr(), harq=None,
                              harq_stride=0, ack=None, iter_max=None, mem=MEM_DEVICE, stream=s)
    _check(L.nrLDPC_hip_dlsch_encode_symbols(C.byref(b), _scr_array(scrambling, len(tbs))), "nrLDPC_hip_dlsch_encode_symbols")


def dlsch_encode_device(tbs, payload, coded, stream=None):
    """payload: torch uint8 [>= tb_layout po[-1]] on the GPU, coded: torch uint8 [>= co[-1]] (out). Asynchronous."""
    import torch
    L = _tb_lib()
    po, co, _, _ = tb_layout(tbs)
    assert payload.is_cuda and coded.is_cuda and payload.numel() >= po[-1] and coded.numel() >= co[-1]
    arr = _tb_array(tbs, po, co, None)
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    b = nrLDPC_hip_tb_batch_t(n_tb=len(tbs), tb=arr, payload=payload.data_ptr(), coded=coded.data_ptr(), harq=None,
                              harq_stride=0, ack=None, iter_max=None, mem=MEM_DEVICE, stream=s)
    _check(L.nrLDPC_hip_dlsch_encode(C.byref(b)), "nrLDPC_hip_dlsch_encode")


def _ptr(x):
    """address of a torch tensor / numpy array / PinnedArray, None for None"""
    if x is None:
        return None
    if isinstance(x, PinnedArray):
        return x.a.ctypes.data
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return x.data_ptr()


class PreparedTbBatch:
    """A transport-block batch descriptor built once and submitted many times (slot after slot with the same
    allocation): keeps the ctypes marshalling out of the caller's per-slot path.  `encode()` / `decode()` are the bare
    C calls nrLDPC_hip_dlsch_encode / nrLDPC_hip_ulsch_decode (asynchronous on the batch's stream with device buffers,
    synchronous with host buffers).  Buffers: torch CUDA tensors (mem = MEM_DEVICE, the default), or numpy arrays /
    PinnedArray objects with mem = MEM_HOST, optionally | MEM_HARQ_DEVICE (harq a CUDA tensor) or | MEM_HARQ_LIBRARY
    (harq None, harq_ids = one id per transport block).  scrambling = one (n_rnti, q, n_id) per transport block: the calls
    are nrLDPC_hip_dlsch_encode_scrambled / nrLDPC_hip_ulsch_decode_scrambled, and an encode's output follows
    tb_layout_packed.  symbols=True (with scrambling): coded_or_llr holds the TBs' symbol records (pack_symbol_records) and
    decode() is nrLDPC_hip_ulsch_decode_symbols; encode() is nrLDPC_hip_dlsch_encode_symbols, its output following
    tb_layout_symbols."""

    def __init__(self, tbs, payload, coded_or_llr, harq=None, ack=None, iter_max=None, numMaxIter=8, stream=None, mem=MEM_DEVICE,
                 harq_ids=None, scrambling=None, symbols=False):
        self._lib = _tb_lib()
        po, co, ho, _ = tb_layout(tbs)
        self.scr = None if scrambling is None else _scr_array(scrambling, len(tbs))
        assert not symbols or self.scr is not None, "symbol records are always scrambled: pass scrambling"
        self.sym = bool(symbols)
        self._coded_packed = tb_layout_packed(tbs)[0]
        self._keep = (payload, coded_or_llr, harq, ack, iter_max)
        if harq_ids is not None:
            assert mem & MEM_HARQ_LIBRARY and len(harq_ids) == len(tbs)
            ho = list(harq_ids)
        self.arr = _tb_array(tbs, po, co, ho if (harq is not None or harq_ids is not None) else None, numMaxIter)
        s = None
        if mem & MEM_DEVICE:
            import torch
            s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        if self.scr is not None:
            self.arr_enc = _tb_array(tbs, po, tb_layout_symbols(tbs)[0] if self.sym else self._coded_packed, None, numMaxIter)
        self.batch = nrLDPC_hip_tb_batch_t(
            n_tb=len(tbs), tb=self.arr, payload=_ptr(payload), coded=_ptr(coded_or_llr),
            harq=_ptr(harq), harq_stride=0 if (harq is None and harq_ids is None) else HARQ_STRIDE,
            ack=_ptr(ack), iter_max=_ptr(iter_max), mem=mem, stream=s)

    def encode(self):
        if self.scr is None:
            _check(self._lib.nrLDPC_hip_dlsch_encode(C.byref(self.batch)), "nrLDPC_hip_dlsch_encode")
        else:
            if not hasattr(self, "batch_enc"):   # (the packed / symbol layout's coded offsets)
                self.batch_enc = nrLDPC_hip_tb_batch_t.from_buffer_copy(self.batch)
                self.batch_enc.tb = self.arr_enc
            if self.sym:
                _check(self._lib.nrLDPC_hip_dlsch_encode_symbols(C.byref(self.batch_enc), self.scr), "nrLDPC_hip_dlsch_encode_symbols")
            else:
                _check(self._lib.nrLDPC_hip_dlsch_encode_scrambled(C.byref(self.batch_enc), self.scr),
                       "nrLDPC_hip_dlsch_encode_scrambled")

    def decode(self):
        _decode_call(self._lib, self.batch, self.scr, self.sym)

    # HIP graphs: capture on the batch's own stream (torch.cuda.graph(g, stream=<the stream the batch was made on>)) after
    # two warm-up calls there; a call whose descriptors repeat only enqueues kernels and memsets.


def ulsch_decode_device(tbs, llr, harq, payload, ack, iter_max, numMaxIter=8, stream=None, harq_ids=None):
    """llr: torch int16 [>= co[-1]], harq: torch int16 [>= ho[-1]], payload: torch uint8 [>= po[-1]] (out),
    ack: torch uint8 [n], iter_max: torch int32 [n].  Asynchronous; tb dicts get their llrLen updated.
    harq=None with harq_ids: the library keeps the soft buffers (MEM_HARQ_LIBRARY)."""
    _ulsch_decode_device(tbs, llr, harq, payload, ack, iter_max, numMaxIter, stream, harq_ids, None)


def ulsch_decode_scrambled_device(tbs, llr, harq, payload, ack, iter_max, scrambling, numMaxIter=8, stream=None, harq_ids=None):
    """ulsch_decode_device on scrambled LLRs (nrLDPC_hip_ulsch_decode_scrambled): scrambling = one (n_rnti, q, n_id) per TB;
    `llr` is only read."""
    _ulsch_decode_device(tbs, llr, harq, payload, ack, iter_max, numMaxIter, stream, harq_ids, _scr_array(scrambling, len(tbs)))


def ulsch_decode_symbols_device(tbs, records, harq, payload, ack, iter_max, scrambling, numMaxIter=8, stream=None, harq_ids=None):
    """ulsch_decode_scrambled_device from symbol records (nrLDPC_hip_ulsch_decode_symbols): `records` = torch int16 [>= co[-1]]
    with TB i's planar record (pack_symbol_records) at tb_layout co[i]; only read."""
    _ulsch_decode_device(tbs, records, harq, payload, ack, iter_max, numMaxIter, stream, harq_ids, _scr_array(scrambling, len(tbs)),
                         sym=True)


def _ulsch_decode_device(tbs, llr, harq, payload, ack, iter_max, numMaxIter, stream, harq_ids, scr, sym=False):
    import torch
    L = _tb_lib()
    po, co, ho, _ = tb_layout(tbs)
    assert llr.is_cuda and llr.dtype == torch.int16
    mem = MEM_DEVICE
    if harq_ids is not None:
        assert harq is None and len(harq_ids) == len(tbs)
        ho, mem = list(harq_ids), MEM_DEVICE | MEM_HARQ_LIBRARY
    else:
        assert harq.dtype == torch.int16 and harq.numel() >= ho[-1]
    arr = _tb_array(tbs, po, co, ho, numMaxIter)
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    b = nrLDPC_hip_tb_batch_t(n_tb=len(tbs), tb=arr, payload=payload.data_ptr(), coded=llr.data_ptr(), harq=_ptr(harq),
                              harq_stride=HARQ_STRIDE, ack=ack.data_ptr(), iter_max=iter_max.data_ptr(), mem=mem,
                              stream=s)
    _decode_call(L, b, scr, sym)
    for i, t in enumerate(tbs):
        t["llrLen"] = arr[i].llrLen


# ---------------------------------------------------------------------------------------------------------
# Codeword scrambling (include/nrLDPC_hip.h: nrLDPC_hip_codeword_scrambling / _unscrambling / nrLDPC_hip_gold_words)
# ---------------------------------------------------------------------------------------------------------
EXPORTS += ["nrLDPC_hip_codeword_scrambling", "nrLDPC_hip_codeword_unscrambling", "nrLDPC_hip_gold_words"]


def _scr_lib():
    L = load_library()
    L.nrLDPC_hip_gold_words.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.nrLDPC_hip_gold_words.restype = C.c_int32
    L.nrLDPC_hip_codeword_scrambling.argtypes = [C.c_void_p, C.c_uint32, C.c_uint8, C.c_uint32, C.c_uint32, C.c_void_p,
                                                 C.c_int32, C.c_void_p]
    L.nrLDPC_hip_codeword_scrambling.restype = C.c_int32
    L.nrLDPC_hip_codeword_unscrambling.argtypes = [C.c_void_p, C.c_uint32, C.c_uint8, C.c_uint32, C.c_uint32, C.c_int32,
                                                   C.c_void_p]
    L.nrLDPC_hip_codeword_unscrambling.restype = C.c_int32
    return L


def gold_c_init(n_rnti, q, n_id):
    """c_init of PDSCH / PUSCH data scrambling (38.211 7.3.1.1 / 6.3.1.1)"""
    return (n_rnti << 15) + (q << 14) + n_id


def gold_words(c_init, first_word, n_words):
    """uint32[n_words]: words first_word .. of the Gold sequence of c_init (bit k of word w = c(32w + k)); host only."""
    out = np.zeros(max(n_words, 1), np.uint32)
    _check(_scr_lib().nrLDPC_hip_gold_words(c_init, first_word, n_words, out.ctypes.data), "nrLDPC_hip_gold_words")
    return out[:n_words]


def _scr_size(size, n):
    """the element count a scrambling call covers: all of the array, or its first `size` elements"""
    n_sz = n if size is None else int(size)
    if not 0 <= n_sz <= n:
        raise ValueError(f"size {n_sz} outside the array's {n} elements")
    return n_sz


def codeword_scrambling(bits, q, n_id, n_rnti, out=None, size=None, stream=None):
    """nr_codeword_scrambling: `bits` one bit per byte, the first `size` of them (all by default).  numpy uint8 -> host call,
    returns uint32[ceil(size/32)]; torch uint8 CUDA tensor -> device call enqueued on `stream` into `out`, a contiguous
    torch int32 / uint32 CUDA tensor of at least that many words on the same GPU; returns `out`."""
    L = _scr_lib()
    if isinstance(bits, np.ndarray):
        assert bits.dtype == np.uint8
        src = np.ascontiguousarray(bits).reshape(-1)
        n = _scr_size(size, src.size)
        res = np.zeros(max((n + 31) // 32, 1), np.uint32)
        _check(L.nrLDPC_hip_codeword_scrambling(src.ctypes.data, n, q, n_id, n_rnti, res.ctypes.data, MEM_HOST, None),
               "nrLDPC_hip_codeword_scrambling")
        return res[:(n + 31) // 32]
    import torch
    assert bits.is_cuda and bits.dtype == torch.uint8 and bits.is_contiguous()
    n = _scr_size(size, bits.numel())
    assert out is not None and out.is_cuda and out.device == bits.device and out.is_contiguous()
    assert out.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)) and out.numel() >= (n + 31) // 32
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    _check(L.nrLDPC_hip_codeword_scrambling(bits.data_ptr(), n, q, n_id, n_rnti, out.data_ptr(), MEM_DEVICE, s),
           "nrLDPC_hip_codeword_scrambling")
    return out


def codeword_unscrambling(llr, q, n_id, n_rnti, size=None, stream=None):
    """nr_codeword_unscrambling, in place on the first `size` int16 LLRs (all by default): numpy -> host call, torch CUDA
    tensor -> device call enqueued on `stream`."""
    L = _scr_lib()
    if isinstance(llr, np.ndarray):
        assert llr.dtype == np.int16 and llr.flags.c_contiguous
        n = _scr_size(size, llr.size)
        _check(L.nrLDPC_hip_codeword_unscrambling(llr.ctypes.data, n, q, n_id, n_rnti, MEM_HOST, None),
               "nrLDPC_hip_codeword_unscrambling")
        return llr
    import torch
    assert llr.is_cuda and llr.dtype == torch.int16 and llr.is_contiguous()
    n = _scr_size(size, llr.numel())
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    _check(L.nrLDPC_hip_codeword_unscrambling(llr.data_ptr(), n, q, n_id, n_rnti, MEM_DEVICE, s),
           "nrLDPC_hip_codeword_unscrambling")
    return llr


# ---------------------------------------------------------------------------------------------------------
# Modulation mapping and soft demapping (include/nrLDPC_hip.h: nrLDPC_hip_mod_table / _modulation / _ulsch_llr)
# ---------------------------------------------------------------------------------------------------------
EXPORTS += ["nrLDPC_hip_mod_table", "nrLDPC_hip_modulation", "nrLDPC_hip_ulsch_llr", "nrLDPC_hip_ulsch_decode_symbols"]


def _qam_lib():
    L = load_library()
    L.nrLDPC_hip_mod_table.argtypes = [C.c_uint8, C.c_void_p]
    L.nrLDPC_hip_mod_table.restype = C.c_int32
    L.nrLDPC_hip_modulation.argtypes = [C.c_void_p, C.c_uint32, C.c_uint8, C.c_void_p, C.c_int32, C.c_void_p]
    L.nrLDPC_hip_modulation.restype = C.c_int32
    L.nrLDPC_hip_ulsch_llr.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_uint8, C.c_void_p, C.c_int32, C.c_void_p]
    L.nrLDPC_hip_ulsch_llr.restype = C.c_int32
    if hasattr(L, "nrLDPC_hip_layer_mapping"):
        L.nrLDPC_hip_layer_mapping.argtypes = [C.c_void_p, C.c_uint32, C.c_uint8, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p]
        L.nrLDPC_hip_layer_mapping.restype = C.c_int32
    return L


def mod_table(Qm):
    """int16[2^Qm, 2]: the (re, im) point of every index of the constellation of Qm (host only)"""
    out = np.zeros((1 << Qm if Qm in (2, 4, 6, 8) else 1, 2), np.int16)
    _check(_qam_lib().nrLDPC_hip_mod_table(Qm, out.ctypes.data), "nrLDPC_hip_mod_table")
    return out


def modulation(words, length, Qm, out=None, stream=None):
    """nr_modulation: `length` bits of packed words (bit k of word w = bit 32w + k) -> length/Qm (re, im) points.  numpy
    uint32 -> host call, returns int16[length/Qm, 2]; torch int32/uint32 CUDA tensor -> device call enqueued on `stream` into
    `out`, a contiguous torch int16 CUDA tensor of at least 2 length/Qm elements on the same GPU; returns `out`."""
    L = _qam_lib()
    n_sym = length // Qm if Qm else 0
    if isinstance(words, np.ndarray):
        assert words.dtype in (np.uint32, np.int32)
        src = np.ascontiguousarray(words).reshape(-1)
        if src.size < (length + 31) // 32:
            raise ValueError(f"{length} bits need {(length + 31) // 32} words, the array has {src.size}")
        res = np.zeros((max(n_sym, 1), 2), np.int16)
        _check(L.nrLDPC_hip_modulation(src.ctypes.data, length, Qm, res.ctypes.data, MEM_HOST, None), "nrLDPC_hip_modulation")
        return res[:n_sym]
    import torch
    assert words.is_cuda and words.is_contiguous() and words.element_size() == 4 and words.numel() >= (length + 31) // 32
    assert out is not None and out.is_cuda and out.device == words.device and out.is_contiguous()
    assert out.dtype == torch.int16 and out.numel() >= 2 * n_sym
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    _check(L.nrLDPC_hip_modulation(words.data_ptr(), length, Qm, out.data_ptr(), MEM_DEVICE, s), "nrLDPC_hip_modulation")
    return out


def _c16_count(a):
    """c16 values in an int16 [n, 2] / [2n] or int32 [n] array or tensor"""
    nb = a.size * a.itemsize if isinstance(a, np.ndarray) else a.numel() * a.element_size()
    assert nb % 4 == 0, "c16 arrays hold whole (re, im) pairs"
    return nb // 4


def ulsch_llr(y, mags, Qm, out=None, stream=None):
    """nr_ulsch_compute_llr for one stream: y = the equalised symbols, mags = (mag_a, mag_b, mag_c)[:Qm/2 - 1], all c16 (int16
    [nb_re, 2] or int32 [nb_re]).  numpy -> host call, returns int16[nb_re * Qm]; torch CUDA tensors (contiguous, one GPU) ->
    device call enqueued on `stream` into `out`, a contiguous torch int16 CUDA tensor of at least nb_re * Qm elements."""
    L = _qam_lib()
    mags = list(mags)
    if len(mags) != max(Qm // 2 - 1, 0):
        raise ValueError(f"Qm {Qm} takes {max(Qm // 2 - 1, 0)} magnitude arrays, got {len(mags)}")
    nb_re = _c16_count(y)
    for m in mags:
        if _c16_count(m) != nb_re:
            raise ValueError("every magnitude array has one c16 value per RE")
    if isinstance(y, np.ndarray):
        arrs = [np.ascontiguousarray(a) for a in [y] + mags]
        for a in arrs:
            assert a.dtype in (np.int16, np.int32)
        ptrs = [a.ctypes.data for a in arrs] + [None] * (4 - len(arrs))
        res = np.zeros(max(nb_re * Qm, 1), np.int16)
        _check(L.nrLDPC_hip_ulsch_llr(*ptrs, nb_re, Qm, res.ctypes.data, MEM_HOST, None), "nrLDPC_hip_ulsch_llr")
        return res[:nb_re * Qm]
    import torch
    arrs = [y] + mags
    for a in arrs:
        assert a.is_cuda and a.is_contiguous() and a.dtype in (torch.int16, torch.int32) and a.device == y.device
    assert out is not None and out.is_cuda and out.device == y.device and out.is_contiguous()
    assert out.dtype == torch.int16 and out.numel() >= nb_re * Qm
    ptrs = [a.data_ptr() for a in arrs] + [None] * (4 - len(arrs))
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    _check(L.nrLDPC_hip_ulsch_llr(*ptrs, nb_re, Qm, out.data_ptr(), MEM_DEVICE, s), "nrLDPC_hip_ulsch_llr")
    return out


def pack_symbol_records(blocks):
    """The planar symbol records of nrLDPC_hip_ulsch_decode_symbols: blocks[i] = (y, mag_a, ...) of one TB, Qm/2 c16 arrays of
    S = G/Qm values each in codeword symbol order (numpy int16 [S, 2] or int32 [S]) -> int16[G] per TB: y's S values, then
    mag_a's, ... (place record i at tb_layout co[i] of the call's array)."""
    out = []
    for planes in blocks:
        ps = [np.ascontiguousarray(p).view(np.int16).reshape(-1) for p in planes]
        if any(p.size != ps[0].size for p in ps):
            raise ValueError("every plane of a record has S c16 values")
        out.append(np.concatenate(ps).astype(np.int16, copy=False))
    return out


# ---------------------------------------------------------------------------------------------------------
# Layer mapping and the DL-SCH chain call to symbols (include/nrLDPC_hip.h: nrLDPC_hip_layer_mapping / _dlsch_encode_symbols)
# ---------------------------------------------------------------------------------------------------------
EXPORTS += ["nrLDPC_hip_layer_mapping", "nrLDPC_hip_dlsch_encode_symbols"]


def layer_mapping(x, Nl, out=None, layer_stride=None, n_symbs=None, stream=None):
    """nr_layer_mapping for one codeword: the first n_symbs (all by default) c16 points of x (int16 [n, 2] / [2n] or int32 [n])
    -> Nl planes, out[l layer_stride + i] = x[Nl i + l] in c16 units (layer_stride = n_symbs / Nl by default).  numpy -> host
    call, returns int16[Nl, layer_stride, 2] (zeros between the planes); torch CUDA tensor -> device call enqueued on `stream`
    into `out`, a contiguous torch CUDA tensor on the same GPU of at least 4 ((Nl - 1) layer_stride + n_symbs / Nl) bytes;
    returns `out`."""
    L = _qam_lib()
    n = _c16_count(x) if n_symbs is None else int(n_symbs)
    stride = n // Nl if (layer_stride is None and Nl) else (layer_stride or 0)
    if isinstance(x, np.ndarray):
        src = np.ascontiguousarray(x)
        res = np.zeros((max(Nl, 1), max(stride, 1), 2), np.int16)
        _check(L.nrLDPC_hip_layer_mapping(src.ctypes.data, n, Nl, res.ctypes.data, stride, MEM_HOST, None), "nrLDPC_hip_layer_mapping")
        return res[:, :stride]
    import torch
    assert x.is_cuda and x.is_contiguous() and out is not None and out.is_cuda and out.is_contiguous() and out.device == x.device
    assert out.numel() * out.element_size() >= 4 * ((Nl - 1) * stride + n // Nl)
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    _check(L.nrLDPC_hip_layer_mapping(x.data_ptr(), n, Nl, out.data_ptr(), stride, MEM_DEVICE, s), "nrLDPC_hip_layer_mapping")
    return out


# ---------------------------------------------------------------------------------------------------------
# UL receive front (include/nrLDPC_hip.h: nrLDPC_hip_ulsch_channel_level / _channel_compensation and their _host mirrors)
# ---------------------------------------------------------------------------------------------------------
EXPORTS += ["nrLDPC_hip_ulsch_channel_level", "nrLDPC_hip_ulsch_channel_compensation", "nrLDPC_hip_ulsch_compensate_host",
            "nrLDPC_hip_ulsch_level_host"]


def _struct_array(T, dicts, keys, bytes_=()):
    """dicts with the fields `keys` of ctypes structure T (a missing one is 0; those in bytes_ are cut to 8 bits, a sequence fills
    an array field) -> T[max(n, 1)]; the library checks the values"""
    arr = (T * max(len(dicts), 1))()
    for i, d in enumerate(dicts):
        for k in keys:
            v = d.get(k, 0)
            if isinstance(v, (list, tuple)):
                v = type(getattr(arr[i], k))(*[x & 0xff for x in (list(v) + [0] * 4)[:4]])
            setattr(arr[i], k, v & 0xff if k in bytes_ else v)
    return arr


def _mem_of(arrays, stream, int32=()):
    """What the slot-level wrappers pass for their arrays: numpy -> HOST mem, torch -> DEVICE mem on `stream` or on the current
    stream.  `arrays` are int16, `int32` arrays int32 (None: not given), all C-contiguous and of one kind -- torch tensors on the GPU
    of the first.  Returns (ptr, numel, mem, stream): ptr(a) = the address of a (None for None), numel(a) = its elements."""
    given = [a for a in tuple(arrays) + tuple(int32) if a is not None]
    if isinstance(arrays[0], np.ndarray):
        assert all(a.dtype == np.int16 and a.flags.c_contiguous for a in arrays)
        assert all(a is None or (a.dtype == np.int32 and a.flags.c_contiguous) for a in int32)
        return (lambda a: None if a is None else a.ctypes.data), (lambda a: a.size), MEM_HOST, None
    import torch
    assert all(a.is_cuda and a.is_contiguous() and a.device == arrays[0].device for a in given)
    assert all(a.dtype == torch.int16 for a in arrays) and all(a is None or a.dtype == torch.int32 for a in int32)
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    return (lambda a: None if a is None else a.data_ptr()), (lambda a: a.numel()), MEM_DEVICE, s


def _level_out(ch, out, n):
    """where a level call writes: numpy -> a new int32[max(n, 1)]; torch -> the caller's `out`, checked"""
    if isinstance(ch, np.ndarray):
        return np.zeros(max(n, 1), np.int32)
    assert out is not None and out.numel() >= n
    return out


class nrLDPC_hip_rx_seg_t(C.Structure):
    _fields_ = [("tb", C.c_uint32), ("Qm", C.c_uint8), ("pad", C.c_uint8 * 3), ("nb_re", C.c_uint32), ("plane", C.c_uint32),
                ("sym_off", C.c_uint32), ("pad2", C.c_uint32), ("rx_off", C.c_uint64), ("ch_off", C.c_uint64), ("rec_off", C.c_uint64)]


def _rxf_lib():
    L = load_library()
    L.nrLDPC_hip_ulsch_channel_level.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(nrLDPC_hip_rx_seg_t), C.c_uint32, C.c_void_p,
                                                 C.c_int32, C.c_void_p]
    L.nrLDPC_hip_ulsch_channel_level.restype = C.c_int32
    L.nrLDPC_hip_ulsch_channel_compensation.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(nrLDPC_hip_rx_seg_t),
                                                        C.c_uint32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.nrLDPC_hip_ulsch_channel_compensation.restype = C.c_int32
    L.nrLDPC_hip_ulsch_compensate_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint8, C.c_int32, C.c_void_p]
    L.nrLDPC_hip_ulsch_compensate_host.restype = C.c_int32
    L.nrLDPC_hip_ulsch_level_host.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
    L.nrLDPC_hip_ulsch_level_host.restype = C.c_int32
    return L


def _rx_seg_array(segs):
    """dicts (tb, Qm, nb_re, plane, sym_off, rx_off, ch_off, rec_off) -> nrLDPC_hip_rx_seg_t[n]; the library checks the values"""
    return _struct_array(nrLDPC_hip_rx_seg_t, segs, ("tb", "Qm", "nb_re", "plane", "sym_off", "rx_off", "ch_off", "rec_off"), ("Qm",))


def rx_front_segments(tbs, nb_re_per_symbol, rec_off=None):
    """The descriptors of the receive front for transport blocks tbs (dicts with G, Qm): nb_re_per_symbol[i] = the data REs
    of TB i's OFDM symbols in time order (they add up to G/Qm).  TB i's record lies at int16 offset rec_off[i] (tb_layout co[i]
    by default: where ulsch_decode_symbols_device reads it, laid out as pack_symbol_records does); the extracted REs and channel
    estimates of one antenna are taken back to back, TB after TB and symbol after symbol.  Returns (segs, first_sym, rec_off,
    n_in): every segment, each TB's first symbol with REs (the measurement symbol), the record offsets, and the c16 values per
    antenna (ant_stride >= n_in)."""
    if rec_off is None:
        rec_off = tb_layout(tbs)[1][:len(tbs)]
    segs, first, at = [], [], 0
    for i, (t, syms) in enumerate(zip(tbs, nb_re_per_symbol)):
        S = t["G"] // t["Qm"]
        if sum(syms) != S:
            raise ValueError(f"TB {i}: the symbols hold {sum(syms)} REs, G/Qm = {S}")
        off = 0
        for nb in syms:
            segs.append(dict(tb=i, Qm=t["Qm"], nb_re=int(nb), plane=S, sym_off=off, rx_off=at, ch_off=at, rec_off=int(rec_off[i])))
            off += nb
            at += nb
        first.append(next(s for s in segs[len(segs) - len(syms):] if s["nb_re"] > 0))
    return segs, first, [int(o) for o in rec_off], at


def ulsch_compensate_host(rx, ch, n_rx, ant_stride, nb_re, Qm, shift):
    """nr_ulsch_channel_compensation for one layer and one segment on the CPU (csrc/nr_rx_front.h, no GPU): rx / ch = numpy int16
    c16 arrays, antenna a's RE r at c16 index a * ant_stride + r.  Returns int16[Qm/2, nb_re, 2]: y, mag_a, mag_b, mag_c."""
    rx, ch = np.ascontiguousarray(rx, np.int16).reshape(-1), np.ascontiguousarray(ch, np.int16).reshape(-1)
    if 1 <= n_rx <= 8:
        assert min(rx.size, ch.size) >= 2 * ((n_rx - 1) * ant_stride + nb_re)
    out = np.zeros((max(Qm // 2, 1) if Qm in (2, 4, 6, 8) else 1, max(nb_re, 1), 2), np.int16)
    _check(_rxf_lib().nrLDPC_hip_ulsch_compensate_host(rx.ctypes.data, ch.ctypes.data, n_rx, ant_stride, nb_re, Qm, shift, out.ctypes.data),
           "nrLDPC_hip_ulsch_compensate_host")
    return out.reshape(-1)[:Qm // 2 * nb_re * 2].reshape(Qm // 2, nb_re, 2)


def ulsch_level_host(ch, n_rx, ant_stride, nb_re):
    """The channel level of one block's measurement symbol on the CPU (no GPU): (log2_maxh, int32[n_rx] averages)."""
    ch = np.ascontiguousarray(ch, np.int16).reshape(-1)
    if 1 <= n_rx <= 8:
        assert ch.size >= 2 * ((n_rx - 1) * ant_stride + nb_re)
    avg, out = np.zeros(8, np.int32), np.zeros(1, np.int32)
    _check(_rxf_lib().nrLDPC_hip_ulsch_level_host(ch.ctypes.data, n_rx, ant_stride, nb_re, avg.ctypes.data, out.ctypes.data),
           "nrLDPC_hip_ulsch_level_host")
    return int(out[0]), avg[:n_rx]


def ulsch_channel_level(ch, n_rx, ant_stride, first_sym, out=None, stream=None):
    """nrLDPC_hip_ulsch_channel_level: first_sym = one descriptor per block (rx_front_segments).  numpy int16 `ch` -> host call,
    returns int32[n_tb]; torch int16 CUDA tensor -> device call enqueued on `stream` into `out`, a torch int32 CUDA tensor of at
    least n_tb elements on the same GPU; returns `out`."""
    n, res = len(first_sym), _level_out(ch, out, len(first_sym))
    ptr, _, mem, s = _mem_of((ch,), stream, (res,))
    _check(_rxf_lib().nrLDPC_hip_ulsch_channel_level(ptr(ch), n_rx, ant_stride, _rx_seg_array(first_sym), n, ptr(res), mem, s),
           "nrLDPC_hip_ulsch_channel_level")
    return res[:n] if mem == MEM_HOST else res


def ulsch_channel_compensation(rx, ch, n_rx, ant_stride, segs, shift, records, stream=None):
    """nrLDPC_hip_ulsch_channel_compensation: segs = the descriptors (rx_front_segments), shift = int32 per block (the output of
    ulsch_channel_level), records = the int16 array the blocks' symbol records lie in, written in place -- only the segments'
    entries.  numpy arrays -> host call; torch CUDA tensors (one GPU, contiguous) -> device call enqueued on `stream`.  Returns
    `records`."""
    if isinstance(rx, np.ndarray):
        shift = np.ascontiguousarray(shift, np.int32)
    ptr, _, mem, s = _mem_of((rx, ch, records), stream, (shift,))
    _check(_rxf_lib().nrLDPC_hip_ulsch_channel_compensation(ptr(rx), ptr(ch), n_rx, ant_stride, _rx_seg_array(segs), len(segs), ptr(shift), ptr(records),
                                                            mem, s), "nrLDPC_hip_ulsch_channel_compensation")
    return records


# ---------------------------------------------------------------------------------------------------------
# UL receive front from the OFDM grid (include/nrLDPC_hip.h: the _grid calls, extract_host, pusch_grid_segments)
# ---------------------------------------------------------------------------------------------------------
EXPORTS += ["nrLDPC_hip_ulsch_channel_level_grid", "nrLDPC_hip_ulsch_channel_compensation_grid", "nrLDPC_hip_ulsch_extract_host",
            "nrLDPC_hip_pusch_grid_segments"]
RXG_FULL, RXG_DMRS1, RXG_DMRS2 = 0, 1, 2
DMRS_SYMBOL_FOLLOW = 255                # alloc["dmrs_symbol"]: every symbol reads the latest DMRS symbol at or before it (chest_time = 0)


class nrLDPC_hip_rx_grid_seg_t(C.Structure):
    _fields_ = [("tb", C.c_uint32), ("Qm", C.c_uint8), ("pattern", C.c_uint8), ("pad", C.c_uint8 * 2), ("nb_re", C.c_uint32),
                ("plane", C.c_uint32), ("sym_off", C.c_uint32), ("fft_size", C.c_uint32), ("start_re", C.c_uint32), ("pad2", C.c_uint32),
                ("rx_off", C.c_uint64), ("ch_off", C.c_uint64), ("rec_off", C.c_uint64)]


class nrLDPC_hip_pusch_alloc_t(C.Structure):
    _fields_ = [("tb", C.c_uint32), ("Qm", C.c_uint8), ("dmrs_config_type", C.c_uint8), ("num_dmrs_cdm_grps_no_data", C.c_uint8),
                ("dmrs_symbol", C.c_uint8), ("fft_size", C.c_uint32), ("first_carrier_offset", C.c_uint32), ("bwp_start", C.c_uint32),
                ("rb_start", C.c_uint32), ("rb_size", C.c_uint32), ("start_symbol", C.c_uint32), ("nr_of_symbols", C.c_uint32),
                ("ul_dmrs_symb_pos", C.c_uint32), ("plane", C.c_uint32), ("pad", C.c_uint32), ("rx_slot_off", C.c_uint64),
                ("ch_off", C.c_uint64), ("rec_off", C.c_uint64)]


_RXG_SEG_KEYS = ("tb", "Qm", "pattern", "nb_re", "plane", "sym_off", "fft_size", "start_re", "rx_off", "ch_off", "rec_off")
_RXG_ALLOC_KEYS = ("tb", "Qm", "dmrs_config_type", "num_dmrs_cdm_grps_no_data", "dmrs_symbol", "fft_size", "first_carrier_offset", "bwp_start",
                   "rb_start", "rb_size", "start_symbol", "nr_of_symbols", "ul_dmrs_symb_pos", "plane", "rx_slot_off", "ch_off", "rec_off")


def _rxg_lib():
    L = load_library()
    P = C.POINTER(nrLDPC_hip_rx_grid_seg_t)
    L.nrLDPC_hip_ulsch_channel_level_grid.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, P, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p]
    L.nrLDPC_hip_ulsch_channel_level_grid.restype = C.c_int32
    L.nrLDPC_hip_ulsch_channel_compensation_grid.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, P, C.c_uint32, C.c_void_p,
                                                             C.c_void_p, C.c_int32, C.c_void_p]
    L.nrLDPC_hip_ulsch_channel_compensation_grid.restype = C.c_int32
    L.nrLDPC_hip_ulsch_extract_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.nrLDPC_hip_ulsch_extract_host.restype = C.c_int32
    L.nrLDPC_hip_pusch_grid_segments.argtypes = [C.POINTER(nrLDPC_hip_pusch_alloc_t), C.c_uint32, P, C.c_uint32, P, C.POINTER(C.c_uint32)]
    L.nrLDPC_hip_pusch_grid_segments.restype = C.c_int32
    return L


def _rx_grid_seg_array(segs):
    """dicts with the fields of nrLDPC_hip_rx_grid_seg_t -> an array of them; the library checks the values"""
    return _struct_array(nrLDPC_hip_rx_grid_seg_t, segs, _RXG_SEG_KEYS, ("Qm", "pattern"))


def _rxg_p(pattern, j):
    return 2 * j + 1 if pattern == RXG_DMRS1 else (6 * (j // 4) + 2 + j % 4 if pattern == RXG_DMRS2 else j)


def _rxg_check_extent(segs, n_rx, rx_stride, ch_stride, rx_len, ch_len, n_ch=None):
    """The calls do not know the arrays' extents; the wrappers do.  rx_len / ch_len in c16, None where an array is not read; n_ch =
    the estimate arrays (n_rx by default; the two-layer receivers read the 2 n_rx (layer, antenna) pairs)."""
    n_ch = n_rx if n_ch is None else n_ch
    for s in segs:
        if s["nb_re"] == 0 or s.get("pattern", 0) > 2 or not 0 <= s["start_re"] < s["fft_size"]:
            continue                                                   # the library names what is wrong with those
        last = _rxg_p(s["pattern"], s["nb_re"] - 1)
        if last >= s["fft_size"]:
            continue
        if ch_len is not None and s["ch_off"] + (n_ch - 1) * ch_stride + last + 1 > ch_len:
            raise ValueError("a segment's channel estimates leave the array")
        if rx_len is not None:
            top = s["start_re"] + last + 1 if s["start_re"] + last < s["fft_size"] else s["fft_size"]
            if s["rx_off"] + (n_rx - 1) * rx_stride + top > rx_len:
                raise ValueError("a segment's REs leave the grid array")


def ulsch_extract_host(rx_sym, ch_sym, pattern, fft_size, start_re, nb_re):
    """nr_ulsch_extract_rbs of one OFDM symbol of one antenna on the CPU (csrc/nr_rx_grid.h, no GPU): rx_sym = int16 [fft_size, 2],
    the symbol of the grid; ch_sym = int16 [>= p(nb_re - 1) + 1, 2], the estimates from PUSCH subcarrier 0.  Returns (rxFext,
    chFext), int16 [nb_re, 2] each."""
    rx_sym, ch_sym = np.ascontiguousarray(rx_sym, np.int16).reshape(-1), np.ascontiguousarray(ch_sym, np.int16).reshape(-1)
    if pattern in (0, 1, 2) and 0 <= start_re < fft_size and nb_re and _rxg_p(pattern, nb_re - 1) < fft_size:
        assert rx_sym.size >= 2 * fft_size and ch_sym.size >= 2 * (_rxg_p(pattern, nb_re - 1) + 1)
    a, b = np.zeros((max(nb_re, 1), 2), np.int16), np.zeros((max(nb_re, 1), 2), np.int16)
    _check(_rxg_lib().nrLDPC_hip_ulsch_extract_host(rx_sym.ctypes.data, ch_sym.ctypes.data, pattern, fft_size, start_re, nb_re, a.ctypes.data,
                                                    b.ctypes.data), "nrLDPC_hip_ulsch_extract_host")
    return a[:nb_re], b[:nb_re]


def pusch_grid_segments(allocs, cap=None):
    """nrLDPC_hip_pusch_grid_segments: allocs = dicts with the fields of nrLDPC_hip_pusch_alloc_t (dmrs_symbol = DMRS_SYMBOL_FOLLOW:
    every symbol reads the latest DMRS symbol at or before it, the reference with chest_time = 0 but for two CDM groups without
    data; 0..13: that symbol's estimates for the whole allocation).  Returns (segs, first_sym),
    lists of dicts with the fields of nrLDPC_hip_rx_grid_seg_t."""
    n, arr = len(allocs), _struct_array(nrLDPC_hip_pusch_alloc_t, allocs, _RXG_ALLOC_KEYS)
    cap = 14 * n if cap is None else cap
    out, first, n_out = (nrLDPC_hip_rx_grid_seg_t * max(cap, 1))(), (nrLDPC_hip_rx_grid_seg_t * max(n, 1))(), C.c_uint32(0)
    _check(_rxg_lib().nrLDPC_hip_pusch_grid_segments(arr, n, out, cap, first, C.byref(n_out)), "nrLDPC_hip_pusch_grid_segments")
    as_dict = lambda g: {k: int(getattr(g, k)) for k in _RXG_SEG_KEYS}
    return [as_dict(out[i]) for i in range(n_out.value)], [as_dict(first[i]) for i in range(n)]


def ulsch_channel_level_grid(ch, n_rx, ch_ant_stride, first_sym, out=None, stream=None):
    """nrLDPC_hip_ulsch_channel_level_grid: ch = the full-width channel estimates, first_sym = one grid descriptor per block
    (pusch_grid_segments).  numpy int16 -> host call, returns int32[n_tb]; torch int16 CUDA tensor -> device call enqueued on
    `stream` into `out` (torch int32 CUDA, >= n_tb elements); returns `out`."""
    n, res = len(first_sym), _level_out(ch, out, len(first_sym))
    ptr, numel, mem, s = _mem_of((ch,), stream, (res,))
    _rxg_check_extent(first_sym, n_rx, 0, ch_ant_stride, None, numel(ch) // 2)
    _check(_rxg_lib().nrLDPC_hip_ulsch_channel_level_grid(ptr(ch), n_rx, ch_ant_stride, _rx_grid_seg_array(first_sym), n, ptr(res), mem, s),
           "nrLDPC_hip_ulsch_channel_level_grid")
    return res[:n] if mem == MEM_HOST else res


def ulsch_channel_compensation_grid(rx, ch, n_rx, rx_ant_stride, ch_ant_stride, segs, shift, records, stream=None):
    """nrLDPC_hip_ulsch_channel_compensation_grid: rx = the OFDM grid, ch = the full-width channel estimates, segs = the grid
    descriptors (pusch_grid_segments); shift and records as ulsch_channel_compensation.  numpy arrays -> host call; torch CUDA
    tensors -> device call enqueued on `stream`.  Returns `records`."""
    if isinstance(rx, np.ndarray):
        shift = np.ascontiguousarray(shift, np.int32)
    ptr, numel, mem, s = _mem_of((rx, ch, records), stream, (shift,))
    _rxg_check_extent(segs, n_rx, rx_ant_stride, ch_ant_stride, numel(rx) // 2, numel(ch) // 2)
    _check(_rxg_lib().nrLDPC_hip_ulsch_channel_compensation_grid(ptr(rx), ptr(ch), n_rx, rx_ant_stride, ch_ant_stride, _rx_grid_seg_array(segs), len(segs),
                                                                 ptr(shift), ptr(records), mem, s), "nrLDPC_hip_ulsch_channel_compensation_grid")
    return records


# ---------------------------------------------------------------------------------------------------------
# Two-layer MMSE receiver for 64QAM / 256QAM (include/nrLDPC_hip.h: the _mmse calls; csrc/nr_rx_mmse.h)
# ---------------------------------------------------------------------------------------------------------
EXPORTS += ["nrLDPC_hip_ulsch_channel_level_grid_mmse", "nrLDPC_hip_ulsch_mmse_2layers_grid", "nrLDPC_hip_ulsch_mmse_2layers_host",
            "nrLDPC_hip_ulsch_level_mmse_host"]


def _rxm_lib():
    L = _rxg_lib()
    P = C.POINTER(nrLDPC_hip_rx_grid_seg_t)
    L.nrLDPC_hip_ulsch_channel_level_grid_mmse.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, P, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int32,
                                                           C.c_void_p]
    L.nrLDPC_hip_ulsch_channel_level_grid_mmse.restype = C.c_int32
    L.nrLDPC_hip_ulsch_mmse_2layers_grid.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, P, C.c_uint32, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_int32, C.c_void_p]
    L.nrLDPC_hip_ulsch_mmse_2layers_grid.restype = C.c_int32
    L.nrLDPC_hip_ulsch_mmse_2layers_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint8, C.c_int32, C.c_uint32,
                                                     C.c_void_p]
    L.nrLDPC_hip_ulsch_mmse_2layers_host.restype = C.c_int32
    L.nrLDPC_hip_ulsch_level_mmse_host.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p]
    L.nrLDPC_hip_ulsch_level_mmse_host.restype = C.c_int32
    return L


def _level_grid_2layers(L, name, ch, n_rx, ch_ant_stride, first_sym, max_ch, out, stream):
    """the level call `name` of a two-layer receiver: the estimates' extent over the 2 n_rx pairs, then the call (a max_ch that is
    None is the library's to refuse)"""
    n, res = len(first_sym), _level_out(ch, out, len(first_sym))
    if isinstance(ch, np.ndarray) and max_ch is not None:
        max_ch = np.ascontiguousarray(max_ch, np.int32)
    ptr, numel, mem, s = _mem_of((ch,), stream, (res,) if max_ch is None else (res, max_ch))
    assert max_ch is None or numel(max_ch) >= n
    _rxg_check_extent(first_sym, 2 * n_rx, 0, ch_ant_stride, None, numel(ch) // 2)
    _check(getattr(L, name)(ptr(ch), n_rx, ch_ant_stride, _rx_grid_seg_array(first_sym), n, None if max_ch is None else ptr(max_ch), ptr(res), mem, s),
           name)
    return res[:n] if mem == MEM_HOST else res


def _rxm_check_records(segs, rec_len):
    """a segment's doubled output range must lie inside `records` (rec_len in int16)"""
    for s in segs:
        if s["nb_re"] and s["Qm"] in (6, 8) and s["rec_off"] + 2 * ((s["Qm"] // 2 - 1) * s["plane"] + 2 * (s["sym_off"] + s["nb_re"])) > rec_len:
            raise ValueError("a segment's entries leave the record array")


def ulsch_mmse_2layers_host(rx, ch, n_rx, ant_stride, nb_re, Qm, shift, nvar):
    """The two-layer MMSE receiver for one segment on the CPU (csrc/nr_rx_mmse.h, no GPU): rx = numpy int16 c16, antenna a's RE r
    at c16 index a * ant_stride + r; ch the same for pair l * n_rx + a.  Returns int16[2, Qm/2, nb_re, 2]: per layer y, mag_a, mag_b,
    mag_c."""
    rx, ch = np.ascontiguousarray(rx, np.int16).reshape(-1), np.ascontiguousarray(ch, np.int16).reshape(-1)
    if n_rx in (2, 4):
        assert rx.size >= 2 * ((n_rx - 1) * ant_stride + nb_re) and ch.size >= 2 * ((2 * n_rx - 1) * ant_stride + nb_re)
    np_ = Qm // 2 if Qm in (6, 8) else 1
    out = np.zeros((2, np_, max(nb_re, 1), 2), np.int16)
    _check(_rxm_lib().nrLDPC_hip_ulsch_mmse_2layers_host(rx.ctypes.data, ch.ctypes.data, n_rx, ant_stride, nb_re, Qm, shift, nvar, out.ctypes.data),
           "nrLDPC_hip_ulsch_mmse_2layers_host")
    return out.reshape(-1)[:2 * np_ * nb_re * 2].reshape(2, np_, nb_re, 2)


def ulsch_level_mmse_host(ch, n_rx, ant_stride, nb_re, max_ch):
    """The channel level of one two-layer block's measurement symbol on the CPU (no GPU): (log2_maxh, int32[2 n_rx] averages)."""
    ch = np.ascontiguousarray(ch, np.int16).reshape(-1)
    if n_rx in (2, 4):
        assert ch.size >= 2 * ((2 * n_rx - 1) * ant_stride + nb_re)
    avg, out = np.zeros(8, np.int32), np.zeros(1, np.int32)
    _check(_rxm_lib().nrLDPC_hip_ulsch_level_mmse_host(ch.ctypes.data, n_rx, ant_stride, nb_re, max_ch, avg.ctypes.data, out.ctypes.data),
           "nrLDPC_hip_ulsch_level_mmse_host")
    return int(out[0]), avg[:2 * n_rx]


def ulsch_channel_level_grid_mmse(ch, n_rx, ch_ant_stride, first_sym, max_ch, out=None, stream=None):
    """nrLDPC_hip_ulsch_channel_level_grid_mmse: ch = the full-width channel estimates of the 2 n_rx (layer, antenna) pairs,
    ch_ant_stride apart; first_sym = one grid descriptor per block; max_ch = int32 per block.  numpy -> host call, returns
    int32[n_tb]; torch CUDA tensors -> device call enqueued on `stream` into `out` (torch int32 CUDA, >= n_tb elements); returns
    `out`."""
    return _level_grid_2layers(_rxm_lib(), "nrLDPC_hip_ulsch_channel_level_grid_mmse", ch, n_rx, ch_ant_stride, first_sym, max_ch, out, stream)


def ulsch_mmse_2layers_grid(rx, ch, n_rx, rx_ant_stride, ch_ant_stride, segs, shift, nvar, records, stream=None):
    """nrLDPC_hip_ulsch_mmse_2layers_grid: rx = the OFDM grid (n_rx antennas), ch = the full-width channel estimates (2 n_rx
    pairs), segs = the grid descriptors (pusch_grid_segments with plane = G/Qm); shift = int32 per block (the output of
    ulsch_channel_level_grid_mmse), nvar = int32 per block holding the uint32 noise variance; records = the int16 array the blocks'
    symbol records lie in, written in place -- only the segments' entries.  numpy arrays -> host call; torch CUDA tensors -> device
    call enqueued on `stream`.  Returns `records`."""
    if isinstance(rx, np.ndarray):
        shift = np.ascontiguousarray(shift, np.int32)
        nvar = np.ascontiguousarray(np.asarray(nvar).astype(np.uint32).view(np.int32))
    ptr, numel, mem, s = _mem_of((rx, ch, records), stream, (shift, nvar))
    _rxg_check_extent(segs, n_rx, rx_ant_stride, ch_ant_stride, numel(rx) // 2, numel(ch) // 2, n_ch=2 * n_rx)
    _rxm_check_records(segs, numel(records))
    _check(_rxm_lib().nrLDPC_hip_ulsch_mmse_2layers_grid(ptr(rx), ptr(ch), n_rx, rx_ant_stride, ch_ant_stride, _rx_grid_seg_array(segs), len(segs),
                                                         ptr(shift), ptr(nvar), ptr(records), mem, s), "nrLDPC_hip_ulsch_mmse_2layers_grid")
    return records


# ---------------------------------------------------------------------------------------------------------
# Two-layer max-log ML receiver for QPSK / 16QAM (include/nrLDPC_hip.h: the _ml calls; csrc/nr_rx_ml.h)
# ---------------------------------------------------------------------------------------------------------
EXPORTS += ["nrLDPC_hip_ulsch_channel_level_grid_ml", "nrLDPC_hip_ulsch_ml_2layers_grid", "nrLDPC_hip_ulsch_ml_2layers_host",
            "nrLDPC_hip_ulsch_level_ml_host"]


def _rxl_lib():
    L = _rxg_lib()
    P = C.POINTER(nrLDPC_hip_rx_grid_seg_t)
    L.nrLDPC_hip_ulsch_channel_level_grid_ml.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, P, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int32,
                                                         C.c_void_p]
    L.nrLDPC_hip_ulsch_channel_level_grid_ml.restype = C.c_int32
    L.nrLDPC_hip_ulsch_ml_2layers_grid.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, P, C.c_uint32, C.c_void_p, C.c_void_p,
                                                   C.c_int32, C.c_void_p]
    L.nrLDPC_hip_ulsch_ml_2layers_grid.restype = C.c_int32
    L.nrLDPC_hip_ulsch_ml_2layers_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint8, C.c_int32, C.c_void_p]
    L.nrLDPC_hip_ulsch_ml_2layers_host.restype = C.c_int32
    L.nrLDPC_hip_ulsch_level_ml_host.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p]
    L.nrLDPC_hip_ulsch_level_ml_host.restype = C.c_int32
    return L


def _rxl_check_llr(segs, llr_len):
    """a segment's write set must lie inside `llr` (llr_len in int16)"""
    for s in segs:
        if s["nb_re"] and s["Qm"] in (2, 4) and s["rec_off"] + 2 * s["Qm"] * (s["sym_off"] + s["nb_re"]) > llr_len:
            raise ValueError("a segment's LLRs leave the array")


def ulsch_ml_2layers_host(rx, ch, n_rx, ant_stride, nb_re, Qm, shift):
    """The two-layer max-log ML receiver for one segment on the CPU (csrc/nr_rx_ml.h, no GPU): rx = numpy int16 c16, antenna a's
    RE r at c16 index a * ant_stride + r; ch the same for pair l * n_rx + a.  Returns int16[nb_re, 2, Qm]: per RE and layer the
    Qm LLRs, the order of the codeword."""
    rx, ch = np.ascontiguousarray(rx, np.int16).reshape(-1), np.ascontiguousarray(ch, np.int16).reshape(-1)
    if 1 <= n_rx <= 8:
        assert rx.size >= 2 * ((n_rx - 1) * ant_stride + nb_re) and ch.size >= 2 * ((2 * n_rx - 1) * ant_stride + nb_re)
    q = Qm if Qm in (2, 4) else 2
    out = np.zeros(max(nb_re, 1) * 2 * q, np.int16)
    _check(_rxl_lib().nrLDPC_hip_ulsch_ml_2layers_host(rx.ctypes.data, ch.ctypes.data, n_rx, ant_stride, nb_re, Qm, shift, out.ctypes.data),
           "nrLDPC_hip_ulsch_ml_2layers_host")
    return out[:nb_re * 2 * q].reshape(nb_re, 2, q)


def ulsch_level_ml_host(ch, n_rx, ant_stride, nb_re, max_ch):
    """The channel level of one two-layer QPSK / 16QAM block's measurement symbol on the CPU (no GPU): (log2_maxh, int32[2 n_rx]
    averages)."""
    ch = np.ascontiguousarray(ch, np.int16).reshape(-1)
    if 1 <= n_rx <= 8:
        assert ch.size >= 2 * ((2 * n_rx - 1) * ant_stride + nb_re)
    avg, out = np.zeros(16, np.int32), np.zeros(1, np.int32)
    _check(_rxl_lib().nrLDPC_hip_ulsch_level_ml_host(ch.ctypes.data, n_rx, ant_stride, nb_re, max_ch, avg.ctypes.data, out.ctypes.data),
           "nrLDPC_hip_ulsch_level_ml_host")
    return int(out[0]), avg[:2 * n_rx]


def ulsch_channel_level_grid_ml(ch, n_rx, ch_ant_stride, first_sym, max_ch, out=None, stream=None):
    """nrLDPC_hip_ulsch_channel_level_grid_ml: the arguments of ulsch_channel_level_grid_mmse; n_rx = 1..8."""
    return _level_grid_2layers(_rxl_lib(), "nrLDPC_hip_ulsch_channel_level_grid_ml", ch, n_rx, ch_ant_stride, first_sym, max_ch, out, stream)


def ulsch_ml_2layers_grid(rx, ch, n_rx, rx_ant_stride, ch_ant_stride, segs, shift, llr, stream=None):
    """nrLDPC_hip_ulsch_ml_2layers_grid: rx = the OFDM grid (n_rx antennas), ch = the full-width channel estimates (2 n_rx pairs),
    segs = the grid descriptors (pusch_grid_segments with plane = G/Qm, rec_off = the block's coded_off); shift = int32 per block
    (the output of ulsch_channel_level_grid_ml); llr = the int16 array ulsch_decode_scrambled reads, written in place -- only the
    segments' entries.  numpy arrays -> host call; torch CUDA tensors -> device call enqueued on `stream`.  Returns `llr`."""
    if isinstance(rx, np.ndarray):
        shift = np.ascontiguousarray(shift, np.int32)
    ptr, numel, mem, s = _mem_of((rx, ch, llr), stream, (shift,))
    _rxg_check_extent(segs, n_rx, rx_ant_stride, ch_ant_stride, numel(rx) // 2, numel(ch) // 2, n_ch=2 * n_rx)
    _rxl_check_llr(segs, numel(llr))
    _check(_rxl_lib().nrLDPC_hip_ulsch_ml_2layers_grid(ptr(rx), ptr(ch), n_rx, rx_ant_stride, ch_ant_stride, _rx_grid_seg_array(segs), len(segs),
                                                       ptr(shift), ptr(llr), mem, s), "nrLDPC_hip_ulsch_ml_2layers_grid")
    return llr


# ---------------------------------------------------------------------------------------------------------
# PUSCH DMRS channel estimation (include/nrLDPC_hip.h: pusch_channel_estimation and its host forms; csrc/nr_chest.h)
# ---------------------------------------------------------------------------------------------------------
EXPORTS += ["nrLDPC_hip_pusch_channel_estimation", "nrLDPC_hip_pusch_chest_host", "nrLDPC_hip_pusch_dmrs_host", "nrLDPC_hip_delay_table_host",
            "nrLDPC_hip_pusch_chest_segments"]
CHEST_TYPE1_INTERP, CHEST_TYPE2_INTERP, CHEST_TYPE1_AVG, CHEST_TYPE2_AVG = 0, 1, 2, 3


class nrLDPC_hip_chest_seg_t(C.Structure):
    _fields_ = [("mode", C.c_uint8), ("port", C.c_uint8), ("pad", C.c_uint8 * 2), ("fft_size", C.c_uint32), ("start_re", C.c_uint32),
                ("rb_size", C.c_uint32), ("dmrs_offset", C.c_uint32), ("c_init", C.c_uint32), ("delay_off", C.c_uint32), ("pad2", C.c_uint32),
                ("rx_off", C.c_uint64), ("ch_off", C.c_uint64)]


class nrLDPC_hip_pusch_chest_cfg_t(C.Structure):
    _fields_ = [("slot", C.c_uint32), ("scid", C.c_uint32), ("dmrs_scrambling_id", C.c_uint32), ("port", C.c_uint32), ("chest_freq", C.c_uint32)]


_CHEST_SEG_KEYS = ("mode", "port", "fft_size", "start_re", "rb_size", "dmrs_offset", "c_init", "delay_off", "rx_off", "ch_off")
_CHEST_CFG_KEYS = ("slot", "scid", "dmrs_scrambling_id", "port", "chest_freq")


def _chest_lib():
    L = load_library()
    P = C.POINTER(nrLDPC_hip_chest_seg_t)
    L.nrLDPC_hip_pusch_channel_estimation.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, P, C.c_uint32, C.c_void_p, C.c_int32,
                                                      C.c_void_p]
    L.nrLDPC_hip_pusch_channel_estimation.restype = C.c_int32
    L.nrLDPC_hip_pusch_chest_host.argtypes = [C.c_void_p, P, C.c_int32, C.c_void_p]
    L.nrLDPC_hip_pusch_chest_host.restype = C.c_int32
    L.nrLDPC_hip_pusch_dmrs_host.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.nrLDPC_hip_pusch_dmrs_host.restype = C.c_int32
    L.nrLDPC_hip_delay_table_host.argtypes = [C.c_uint32, C.c_int32, C.c_void_p]
    L.nrLDPC_hip_delay_table_host.restype = C.c_int32
    L.nrLDPC_hip_pusch_chest_segments.argtypes = [C.POINTER(nrLDPC_hip_pusch_alloc_t), C.POINTER(nrLDPC_hip_pusch_chest_cfg_t), C.c_uint32, C.c_uint32, P,
                                                  C.c_uint32, C.POINTER(C.c_uint32)]
    L.nrLDPC_hip_pusch_chest_segments.restype = C.c_int32
    return L


def _chest_seg_array(segs):
    """dicts with the fields of nrLDPC_hip_chest_seg_t -> an array of them; the library checks the values"""
    return _struct_array(nrLDPC_hip_chest_seg_t, segs, _CHEST_SEG_KEYS, ("mode", "port"))


def _chest_check_extent(segs, n_rx, rx_stride, ch_stride, rx_len, ch_len, delay_len):
    """The call does not know the arrays' extents; the wrappers do.  Lengths in c16 (rx, ch) and int32 (delay, None = no array)."""
    for s in segs:
        if s["rb_size"] == 0 or 12 * s["rb_size"] > s["fft_size"]:
            continue                                                   # the library names what is wrong with those
        if s["rx_off"] + (n_rx - 1) * rx_stride + s["fft_size"] > rx_len:
            raise ValueError("a descriptor's OFDM symbol leaves the grid array")
        if s["ch_off"] + (n_rx - 1) * ch_stride + 12 * s["rb_size"] > ch_len:
            raise ValueError("a descriptor's channel estimates leave the array")
        if delay_len is not None and s.get("delay_off", 0) + n_rx > delay_len:
            raise ValueError("a descriptor's delays leave the est_delay array")


def delay_table_host(fft_size, delay):
    """Row get_delay_idx(delay) of the delay table of fft_size: int16 [fft_size, 2]."""
    out = np.zeros((max(fft_size, 1), 2), np.int16)
    _check(_chest_lib().nrLDPC_hip_delay_table_host(fft_size, delay, out.ctypes.data), "nrLDPC_hip_delay_table_host")
    return out


def pusch_dmrs_host(c_init, dmrs_offset, n, port, dmrs_type):
    """n conjugated PUSCH DMRS pilots from sequence symbol dmrs_offset on (dmrs_type 0: type 1, 1: type 2): int16 [n, 2]."""
    out = np.zeros((max(n, 1), 2), np.int16)
    _check(_chest_lib().nrLDPC_hip_pusch_dmrs_host(c_init, dmrs_offset, n, port, dmrs_type, out.ctypes.data), "nrLDPC_hip_pusch_dmrs_host")
    return out[:n]


def pusch_chest_host(rx, seg, est_delay, ch):
    """nrLDPC_hip_pusch_chest_host: one descriptor, antenna 0, on the CPU (csrc/nr_chest.h, no GPU).  rx = int16 grid, ch = int16
    estimates (written in place at seg's ch_off).  Returns ch."""
    assert rx.dtype == np.int16 and ch.dtype == np.int16 and rx.flags.c_contiguous and ch.flags.c_contiguous
    _chest_check_extent([seg], 1, 0, 0, rx.size // 2, ch.size // 2, None)
    arr = _chest_seg_array([seg])
    _check(_chest_lib().nrLDPC_hip_pusch_chest_host(rx.ctypes.data, arr, est_delay, ch.ctypes.data), "nrLDPC_hip_pusch_chest_host")
    return ch


def pusch_chest_segments(allocs, cfgs, n_rx, cap=None):
    """nrLDPC_hip_pusch_chest_segments: allocs = dicts with the fields of nrLDPC_hip_pusch_alloc_t, cfgs = parallel dicts with slot,
    scid, dmrs_scrambling_id, port, chest_freq.  Returns a list of dicts with the fields of nrLDPC_hip_chest_seg_t."""
    n = len(allocs)
    assert len(cfgs) == n
    arr, carr = _struct_array(nrLDPC_hip_pusch_alloc_t, allocs, _RXG_ALLOC_KEYS), _struct_array(nrLDPC_hip_pusch_chest_cfg_t, cfgs, _CHEST_CFG_KEYS)
    cap = 14 * n if cap is None else cap
    out, n_out = (nrLDPC_hip_chest_seg_t * max(cap, 1))(), C.c_uint32(0)
    _check(_chest_lib().nrLDPC_hip_pusch_chest_segments(arr, carr, n, n_rx, out, cap, C.byref(n_out)), "nrLDPC_hip_pusch_chest_segments")
    return [{k: int(getattr(out[i], k)) for k in _CHEST_SEG_KEYS} for i in range(n_out.value)]


def pusch_channel_estimation(rx, rx_ant_stride, ch, ch_ant_stride, n_rx, segs, est_delay=None, stream=None):
    """nrLDPC_hip_pusch_channel_estimation: rx = the OFDM grid, ch = the full-width channel estimates (written), segs = the
    descriptors (pusch_chest_segments), est_delay = int32 per (descriptor, antenna) or None (0 everywhere).  numpy int16 arrays
    -> host call; torch int16 CUDA tensors -> device call enqueued on `stream`.  Returns ch."""
    if isinstance(rx, np.ndarray) and est_delay is not None:
        est_delay = np.ascontiguousarray(est_delay, np.int32)
    ptr, numel, mem, s = _mem_of((rx, ch), stream, (est_delay,))
    _chest_check_extent(segs, n_rx, rx_ant_stride, ch_ant_stride, numel(rx) // 2, numel(ch) // 2, None if est_delay is None else numel(est_delay))
    _check(_chest_lib().nrLDPC_hip_pusch_channel_estimation(ptr(rx), rx_ant_stride, ptr(ch), ch_ant_stride, n_rx, _chest_seg_array(segs), len(segs),
                                                            ptr(est_delay), mem, s), "nrLDPC_hip_pusch_channel_estimation")
    return ch


# ---------------------------------------------------------------------------------------------------------
# The estimator's max_ch / nvar and the time average of its estimates (include/nrLDPC_hip.h: pusch_channel_estimation_meas,
# pusch_chest_time_avg and their host forms; csrc/nr_chest.h)
# ---------------------------------------------------------------------------------------------------------
EXPORTS += ["nrLDPC_hip_pusch_channel_estimation_meas", "nrLDPC_hip_pusch_chest_meas_host", "nrLDPC_hip_pusch_chest_time_avg",
            "nrLDPC_hip_pusch_chest_time_avg_host", "nrLDPC_hip_pusch_chest_avg_segments"]


class nrLDPC_hip_chest_avg_seg_t(C.Structure):
    _fields_ = [("ch_off", C.c_uint64 * 4), ("n_sym", C.c_uint32), ("rb_size", C.c_uint32)]


def _chest_meas_lib():
    L = _chest_lib()
    P, A = C.POINTER(nrLDPC_hip_chest_seg_t), C.POINTER(nrLDPC_hip_chest_avg_seg_t)
    U = C.POINTER(C.c_uint32)
    L.nrLDPC_hip_pusch_channel_estimation_meas.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, P, C.c_uint32, C.c_void_p, U, U,
                                                           C.c_uint32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.nrLDPC_hip_pusch_channel_estimation_meas.restype = C.c_int32
    L.nrLDPC_hip_pusch_chest_meas_host.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, P, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), U]
    L.nrLDPC_hip_pusch_chest_meas_host.restype = C.c_int32
    L.nrLDPC_hip_pusch_chest_time_avg.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, A, C.c_uint32, C.c_int32, C.c_void_p]
    L.nrLDPC_hip_pusch_chest_time_avg.restype = C.c_int32
    L.nrLDPC_hip_pusch_chest_time_avg_host.argtypes = [C.c_void_p, A]
    L.nrLDPC_hip_pusch_chest_time_avg_host.restype = C.c_int32
    L.nrLDPC_hip_pusch_chest_avg_segments.argtypes = [C.POINTER(nrLDPC_hip_pusch_alloc_t), C.c_uint32, A, C.c_uint32, U, C.POINTER(C.c_uint8)]
    L.nrLDPC_hip_pusch_chest_avg_segments.restype = C.c_int32
    return L


def _chest_avg_seg_array(segs):
    """dicts with ch_off (a sequence of up to four c16 offsets), n_sym, rb_size -> an array of nrLDPC_hip_chest_avg_seg_t"""
    arr = (nrLDPC_hip_chest_avg_seg_t * max(len(segs), 1))()
    for i, d in enumerate(segs):
        for k, v in enumerate(list(d["ch_off"])[:4]):
            arr[i].ch_off[k] = v
        arr[i].n_sym, arr[i].rb_size = d["n_sym"], d["rb_size"]
    return arr


def _chest_avg_check_extent(segs, n_plane, ch_stride, ch_len):
    for s in segs:
        if not 1 <= s["n_sym"] <= 4 or s["rb_size"] == 0 or len(s["ch_off"]) < s["n_sym"]:
            continue                                                   # the library names what is wrong with those
        if max(s["ch_off"][:s["n_sym"]]) + (n_plane - 1) * ch_stride + 12 * s["rb_size"] > ch_len:
            raise ValueError("a descriptor's channel estimates leave the array")


def _u32_array(values):
    return (C.c_uint32 * max(len(values), 1))(*[int(v) for v in values])


def pusch_channel_estimation_meas(rx, rx_ant_stride, ch, ch_ant_stride, n_rx, segs, seg_tb, nvar_div, est_delay=None, max_ch=None, nvar=None,
                                  stream=None):
    """nrLDPC_hip_pusch_channel_estimation_meas: pusch_channel_estimation that also forms max_ch / nvar per block.  seg_tb = the block
    of each descriptor, nvar_div = nr_of_symbols * nrOfLayers * n_rx per block (both host sequences).  numpy int16 arrays -> host
    call, returns (ch, max_ch int32[n_tb], nvar uint32[n_tb]); torch int16 CUDA tensors -> device call enqueued on `stream` into
    `max_ch` / `nvar` (torch int32 CUDA, >= n_tb elements; nvar holds the uint32), returns (ch, max_ch, nvar)."""
    n_tb = len(nvar_div)
    assert len(seg_tb) == len(segs)
    host = isinstance(rx, np.ndarray)
    if host:
        if est_delay is not None:
            est_delay = np.ascontiguousarray(est_delay, np.int32)
        max_ch, nvar_i = np.zeros(max(n_tb, 1), np.int32), np.zeros(max(n_tb, 1), np.int32)
    else:
        assert max_ch is not None and nvar is not None and max_ch.numel() >= n_tb and nvar.numel() >= n_tb
        nvar_i = nvar
    ptr, numel, mem, s = _mem_of((rx, ch), stream, (est_delay, max_ch, nvar_i))
    _chest_check_extent(segs, n_rx, rx_ant_stride, ch_ant_stride, numel(rx) // 2, numel(ch) // 2, None if est_delay is None else numel(est_delay))
    _check(_chest_meas_lib().nrLDPC_hip_pusch_channel_estimation_meas(ptr(rx), rx_ant_stride, ptr(ch), ch_ant_stride, n_rx, _chest_seg_array(segs),
                                                                      len(segs), ptr(est_delay), _u32_array(seg_tb), _u32_array(nvar_div), n_tb,
                                                                      ptr(max_ch), ptr(nvar_i), mem, s), "nrLDPC_hip_pusch_channel_estimation_meas")
    return (ch, max_ch[:n_tb], nvar_i[:n_tb].view(np.uint32)) if host else (ch, max_ch, nvar)


def pusch_chest_meas_host(rx, rx_ant_stride, n_rx, seg, est_delay=None):
    """nrLDPC_hip_pusch_chest_meas_host: one descriptor over n_rx antennas on the CPU (csrc/nr_chest.h, no GPU).  rx = int16 grid,
    est_delay = int32 array indexed from seg's delay_off, or None.  Returns (max_ch, noise_amp2, nest_count) as Python ints."""
    assert rx.dtype == np.int16 and rx.flags.c_contiguous
    if est_delay is not None:
        est_delay = np.ascontiguousarray(est_delay, np.int32)
    _chest_check_extent([dict(seg, ch_off=0)], n_rx, rx_ant_stride, 0, rx.size // 2, 1 << 62, None if est_delay is None else est_delay.size)
    mx, noise, nest = C.c_int32(0), C.c_uint64(0), C.c_uint32(0)
    _check(_chest_meas_lib().nrLDPC_hip_pusch_chest_meas_host(rx.ctypes.data, rx_ant_stride, n_rx, _chest_seg_array([seg]),
                                                              None if est_delay is None else est_delay.ctypes.data, C.byref(mx), C.byref(noise),
                                                              C.byref(nest)), "nrLDPC_hip_pusch_chest_meas_host")
    return mx.value, noise.value, nest.value


def pusch_chest_time_avg(ch, ch_ant_stride, n_plane, segs, stream=None):
    """nrLDPC_hip_pusch_chest_time_avg: ch = the full-width channel estimates, averaged in place over each descriptor's DMRS symbols
    into its first (segs: dicts with ch_off, n_sym, rb_size; pusch_chest_avg_segments derives them).  numpy int16 -> host call;
    torch int16 CUDA -> device call enqueued on `stream`.  Returns ch."""
    ptr, numel, mem, s = _mem_of((ch,), stream)
    _chest_avg_check_extent(segs, n_plane, ch_ant_stride, numel(ch) // 2)
    _check(_chest_meas_lib().nrLDPC_hip_pusch_chest_time_avg(ptr(ch), ch_ant_stride, n_plane, _chest_avg_seg_array(segs), len(segs), mem, s),
           "nrLDPC_hip_pusch_chest_time_avg")
    return ch


def pusch_chest_time_avg_host(ch, seg):
    """nrLDPC_hip_pusch_chest_time_avg_host: one descriptor, one plane, on the CPU (no GPU), in place.  Returns ch."""
    assert ch.dtype == np.int16 and ch.flags.c_contiguous
    _chest_avg_check_extent([seg], 1, 0, ch.size // 2)
    _check(_chest_meas_lib().nrLDPC_hip_pusch_chest_time_avg_host(ch.ctypes.data, _chest_avg_seg_array([seg])), "nrLDPC_hip_pusch_chest_time_avg_host")
    return ch


def pusch_chest_avg_segments(allocs, cap=None):
    """nrLDPC_hip_pusch_chest_avg_segments: allocs = dicts with the fields of nrLDPC_hip_pusch_alloc_t.  Returns (segs, first_dmrs):
    one dict with ch_off, n_sym, rb_size and the first DMRS symbol per allocation."""
    n = len(allocs)
    arr = _struct_array(nrLDPC_hip_pusch_alloc_t, allocs, _RXG_ALLOC_KEYS)
    cap = n if cap is None else cap
    out, n_out, first = (nrLDPC_hip_chest_avg_seg_t * max(cap, 1))(), C.c_uint32(0), (C.c_uint8 * max(n, 1))()
    _check(_chest_meas_lib().nrLDPC_hip_pusch_chest_avg_segments(arr, n, out, cap, C.byref(n_out), first), "nrLDPC_hip_pusch_chest_avg_segments")
    segs = [dict(ch_off=[int(out[i].ch_off[k]) for k in range(out[i].n_sym)], n_sym=int(out[i].n_sym), rb_size=int(out[i].rb_size))
            for i in range(n_out.value)]
    return segs, [int(first[i]) for i in range(n_out.value)]


# ---------------------------------------------------------------------------------------------------------
# The PUSCH delay search (include/nrLDPC_hip.h: pusch_est_delay and its host form; csrc/nr_delay.h)
# ---------------------------------------------------------------------------------------------------------
EXPORTS += ["nrLDPC_hip_pusch_est_delay", "nrLDPC_hip_pusch_est_delay_host"]
DELAY_RUNNING_MAX, DELAY_PER_ANTENNA = 0, 1


def _delay_lib():
    L = _chest_lib()
    P = C.POINTER(nrLDPC_hip_chest_seg_t)
    L.nrLDPC_hip_pusch_est_delay.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, P, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.nrLDPC_hip_pusch_est_delay.restype = C.c_int32
    L.nrLDPC_hip_pusch_est_delay_host.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, P, C.c_uint32, C.c_void_p, C.c_void_p]
    L.nrLDPC_hip_pusch_est_delay_host.restype = C.c_int32
    return L


def _delay_len(segs, n_rx):
    return max([s.get("delay_off", 0) + n_rx for s in segs] + [1])


def pusch_est_delay(rx, rx_ant_stride, n_rx, segs, flags=DELAY_RUNNING_MAX, est_delay=None, peak=None, stream=None):
    """nrLDPC_hip_pusch_est_delay: rx = the OFDM grid, segs = the estimation's descriptors.  numpy int16 -> host call, returns
    (est_delay int32, peak float32), each as long as the descriptors' delay_off + n_rx reach; torch int16 CUDA -> device call
    enqueued on `stream` into `est_delay` (torch int32 CUDA, the array the estimation calls read) and, where given, `peak` (torch
    float32 CUDA), returns (est_delay, peak)."""
    n = _delay_len(segs, n_rx)
    if isinstance(rx, np.ndarray):
        assert rx.dtype == np.int16 and rx.flags.c_contiguous
        est_delay, peak = np.zeros(n, np.int32), np.zeros(n, np.float32)
        ptr_d, ptr_p, mem, s, rx_len, rx_ptr = est_delay.ctypes.data, peak.ctypes.data, MEM_HOST, None, rx.size // 2, rx.ctypes.data
    else:
        import torch
        ptr, numel, mem, s = _mem_of((rx,), stream, (est_delay,))
        assert est_delay is not None and est_delay.numel() >= n
        assert peak is None or (peak.is_cuda and peak.dtype == torch.float32 and peak.is_contiguous() and peak.device == rx.device and peak.numel() >= n)
        ptr_d, ptr_p, rx_len, rx_ptr = est_delay.data_ptr(), None if peak is None else peak.data_ptr(), rx.numel() // 2, rx.data_ptr()
    _chest_check_extent([dict(g, ch_off=0) for g in segs], n_rx, rx_ant_stride, 0, rx_len, 1 << 62, None)
    _check(_delay_lib().nrLDPC_hip_pusch_est_delay(rx_ptr, rx_ant_stride, n_rx, _chest_seg_array(segs), len(segs), flags, ptr_d, ptr_p, mem, s),
           "nrLDPC_hip_pusch_est_delay")
    return est_delay, peak


def pusch_est_delay_host(rx, rx_ant_stride, n_rx, seg, flags=DELAY_RUNNING_MAX):
    """nrLDPC_hip_pusch_est_delay_host: one descriptor over n_rx antennas on the CPU (csrc/nr_delay.h, no GPU).  Returns (est_delay
    int32[n_rx], peak float32[n_rx]) of the descriptor's antennas."""
    assert rx.dtype == np.int16 and rx.flags.c_contiguous
    _chest_check_extent([dict(seg, ch_off=0)], n_rx, rx_ant_stride, 0, rx.size // 2, 1 << 62, None)
    n = _delay_len([seg], n_rx)
    d, p = np.zeros(n, np.int32), np.zeros(n, np.float32)
    _check(_delay_lib().nrLDPC_hip_pusch_est_delay_host(rx.ctypes.data, rx_ant_stride, n_rx, _chest_seg_array([seg]), flags, d.ctypes.data, p.ctypes.data),
           "nrLDPC_hip_pusch_est_delay_host")
    o = seg.get("delay_off", 0)
    return d[o:o + n_rx], p[o:o + n_rx]


# ---------------------------------------------------------------------------------------------------------
# PDSCH resource mapping with DMRS (include/nrLDPC_hip.h: pdsch_resource_mapping and its host forms; csrc/nr_pdsch_map.h)
# ---------------------------------------------------------------------------------------------------------
EXPORTS += ["nrLDPC_hip_pdsch_resource_mapping", "nrLDPC_hip_pdsch_map_host", "nrLDPC_hip_pdsch_dmrs_host", "nrLDPC_hip_pdsch_map_segments"]
PDM_FULL, PDM_DMRS1, PDM_DMRS2 = 0, 1, 2


class nrLDPC_hip_pdsch_map_seg_t(C.Structure):
    _fields_ = [("pattern", C.c_uint8), ("Nl", C.c_uint8), ("ncdm", C.c_uint8), ("l_prime", C.c_uint8), ("port", C.c_uint8 * 4), ("amp", C.c_int16),
                ("pad", C.c_uint16), ("fft_size", C.c_uint32), ("start_re", C.c_uint32), ("rb_size", C.c_uint32), ("nb_re", C.c_uint32),
                ("sym_off", C.c_uint32), ("plane", C.c_uint32), ("dmrs_offset", C.c_uint32), ("c_init", C.c_uint32), ("pad2", C.c_uint32),
                ("tx_off", C.c_uint64), ("lay_off", C.c_uint64)]


class nrLDPC_hip_pdsch_alloc_t(C.Structure):
    _fields_ = [("Nl", C.c_uint32), ("plane", C.c_uint32), ("dmrs_config_type", C.c_uint32), ("num_dmrs_cdm_grps_no_data", C.c_uint32),
                ("dmrs_ports", C.c_uint32), ("scid", C.c_uint32), ("dl_dmrs_scrambling_id", C.c_uint32), ("slot", C.c_uint32), ("si_rnti", C.c_uint32),
                ("amp", C.c_int32), ("fft_size", C.c_uint32), ("first_carrier_offset", C.c_uint32), ("bwp_start", C.c_uint32), ("rb_start", C.c_uint32),
                ("rb_size", C.c_uint32), ("start_symbol", C.c_uint32), ("nr_of_symbols", C.c_uint32), ("dl_dmrs_symb_pos", C.c_uint32),
                ("tx_slot_off", C.c_uint64), ("lay_off", C.c_uint64)]


_PDM_SEG_KEYS = ("pattern", "Nl", "ncdm", "l_prime", "port", "amp", "fft_size", "start_re", "rb_size", "nb_re", "sym_off", "plane", "dmrs_offset",
                 "c_init", "tx_off", "lay_off")
_PDM_ALLOC_KEYS = tuple(f[0] for f in nrLDPC_hip_pdsch_alloc_t._fields_)


def _pdm_lib():
    L = load_library()
    P = C.POINTER(nrLDPC_hip_pdsch_map_seg_t)
    L.nrLDPC_hip_pdsch_resource_mapping.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, P, C.c_uint32, C.c_int32, C.c_void_p]
    L.nrLDPC_hip_pdsch_resource_mapping.restype = C.c_int32
    L.nrLDPC_hip_pdsch_map_host.argtypes = [C.c_void_p, P, C.c_int32, C.c_void_p]
    L.nrLDPC_hip_pdsch_map_host.restype = C.c_int32
    L.nrLDPC_hip_pdsch_dmrs_host.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.nrLDPC_hip_pdsch_dmrs_host.restype = C.c_int32
    L.nrLDPC_hip_pdsch_map_segments.argtypes = [C.POINTER(nrLDPC_hip_pdsch_alloc_t), C.c_uint32, P, C.c_uint32, C.POINTER(C.c_uint32)]
    L.nrLDPC_hip_pdsch_map_segments.restype = C.c_int32
    return L


def _pdm_seg_array(segs):
    """dicts with the fields of nrLDPC_hip_pdsch_map_seg_t (port = a sequence of up to 4) -> an array of them; the library checks the
    values"""
    return _struct_array(nrLDPC_hip_pdsch_map_seg_t, segs, _PDM_SEG_KEYS, ("pattern", "Nl", "ncdm", "l_prime"))


def _pdm_check_extent(segs, n_tx, tx_stride, lay_len, tx_len):
    """The calls do not know the arrays' extents; the wrappers do.  Lengths in c16."""
    for s in segs:
        if s["rb_size"] == 0 or 12 * s["rb_size"] > s["fft_size"] or not 1 <= s.get("Nl", 0) <= 4 or s["lay_off"] & 1:
            continue                                                   # the library names what is wrong with those
        if s["tx_off"] + (n_tx - 1) * tx_stride + min(s["start_re"] + 12 * s["rb_size"], s["fft_size"]) > tx_len:
            raise ValueError("a descriptor's OFDM symbol leaves the grid array")
        if lay_len is not None and s["lay_off"] // 2 + (s["Nl"] - 1) * s["plane"] + s["sym_off"] + s["nb_re"] > lay_len:
            raise ValueError("a descriptor's layer entries leave the layers array")


def pdsch_dmrs_host(c_init, dmrs_offset, n):
    """n unconjugated PDSCH DMRS pilots (before Wt Wf amp) from sequence symbol dmrs_offset on: int16 [n, 2]."""
    out = np.zeros((max(n, 1), 2), np.int16)
    _check(_pdm_lib().nrLDPC_hip_pdsch_dmrs_host(c_init, dmrs_offset, n, out.ctypes.data), "nrLDPC_hip_pdsch_dmrs_host")
    return out[:n]


def pdsch_map_host(layers, seg, layer, tx):
    """nrLDPC_hip_pdsch_map_host: one descriptor, one antenna, on the CPU (csrc/nr_pdsch_map.h, no GPU).  layers = int16 layer planes,
    layer = 0 .. Nl - 1 or negative for the zeros of an antenna behind the layers, tx = int16 grid (written in place at seg's tx_off).
    Returns tx."""
    assert layers.dtype == np.int16 and tx.dtype == np.int16 and layers.flags.c_contiguous and tx.flags.c_contiguous
    _pdm_check_extent([seg], 1, 0, layers.size // 2, tx.size // 2)
    _check(_pdm_lib().nrLDPC_hip_pdsch_map_host(layers.ctypes.data, _pdm_seg_array([seg]), layer, tx.ctypes.data), "nrLDPC_hip_pdsch_map_host")
    return tx


def pdsch_map_segments(allocs, cap=None):
    """nrLDPC_hip_pdsch_map_segments: allocs = dicts with the fields of nrLDPC_hip_pdsch_alloc_t.  Returns a list of dicts with the
    fields of nrLDPC_hip_pdsch_map_seg_t."""
    n, arr = len(allocs), _struct_array(nrLDPC_hip_pdsch_alloc_t, allocs, _PDM_ALLOC_KEYS)
    cap = 14 * n if cap is None else cap
    out, n_out = (nrLDPC_hip_pdsch_map_seg_t * max(cap, 1))(), C.c_uint32(0)
    _check(_pdm_lib().nrLDPC_hip_pdsch_map_segments(arr, n, out, cap, C.byref(n_out)), "nrLDPC_hip_pdsch_map_segments")
    return [{k: (list(out[i].port) if k == "port" else int(getattr(out[i], k))) for k in _PDM_SEG_KEYS} for i in range(n_out.value)]


def pdsch_resource_mapping(layers, tx, tx_ant_stride, n_tx, segs, stream=None):
    """nrLDPC_hip_pdsch_resource_mapping: layers = the layer planes (dlsch_encode_symbols output), tx = the transmit grid (written),
    segs = the descriptors (pdsch_map_segments).  numpy int16 arrays -> host call; torch int16 CUDA tensors -> device call enqueued
    on `stream`.  Returns tx."""
    ptr, numel, mem, s = _mem_of((tx, layers), stream)
    _pdm_check_extent(segs, n_tx, tx_ant_stride, numel(layers) // 2, numel(tx) // 2)
    _check(_pdm_lib().nrLDPC_hip_pdsch_resource_mapping(ptr(layers), ptr(tx), tx_ant_stride, n_tx, _pdm_seg_array(segs), len(segs), mem, s),
           "nrLDPC_hip_pdsch_resource_mapping")
    return tx


# ---------------------------------------------------------------------------------------------------------
# PDSCH resource mapping with precoding (include/nrLDPC_hip.h: pdsch_resource_mapping_precoded and its host forms)
# ---------------------------------------------------------------------------------------------------------
EXPORTS += ["nrLDPC_hip_pdsch_resource_mapping_precoded", "nrLDPC_hip_pdsch_precode_host", "nrLDPC_hip_pdsch_precode_segments"]


class nrLDPC_hip_pm_pdu_t(C.Structure):
    _fields_ = [("pm_idx", C.c_uint16), ("numLayers", C.c_uint16), ("num_ant_ports", C.c_uint16), ("pad", C.c_uint16),
                ("weights", C.c_int16 * 2 * 8 * 4)]


class nrLDPC_hip_pdsch_prg_t(C.Structure):
    _fields_ = [("prg_size", C.c_uint32), ("pmi_off", C.c_uint32), ("pmi_count", C.c_uint32)]


_PDM_PRG_KEYS = ("prg_size", "pmi_off", "pmi_count")


def _pre_lib():
    L = _pdm_lib()
    S, A, G, M = (C.POINTER(nrLDPC_hip_pdsch_map_seg_t), C.POINTER(nrLDPC_hip_pdsch_alloc_t), C.POINTER(nrLDPC_hip_pdsch_prg_t),
                  C.POINTER(nrLDPC_hip_pm_pdu_t))
    L.nrLDPC_hip_pdsch_resource_mapping_precoded.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, S, G, C.c_uint32, C.c_void_p, C.c_uint32, M,
                                                             C.c_uint32, C.c_int32, C.c_void_p]
    L.nrLDPC_hip_pdsch_resource_mapping_precoded.restype = C.c_int32
    L.nrLDPC_hip_pdsch_precode_host.argtypes = [C.c_void_p, S, G, C.c_void_p, C.c_uint32, M, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.nrLDPC_hip_pdsch_precode_host.restype = C.c_int32
    L.nrLDPC_hip_pdsch_precode_segments.argtypes = [A, G, C.c_uint32, C.c_uint32, S, G, C.c_uint32, C.POINTER(C.c_uint32)]
    L.nrLDPC_hip_pdsch_precode_segments.restype = C.c_int32
    return L


def pdsch_pm_table(mats):
    """The precoding-matrix table: dicts with pm_idx, numLayers, num_ant_ports and weights = int16 [layers <= 4][ports <= 8][2]
    (Re, Im; what is not given is 0) -> (array of nrLDPC_hip_pm_pdu_t or None, n).  None / an empty list: no table."""
    if not mats:
        return None, 0
    arr = (nrLDPC_hip_pm_pdu_t * len(mats))()
    for i, d in enumerate(mats):
        arr[i].pm_idx, arr[i].numLayers, arr[i].num_ant_ports = d["pm_idx"], d["numLayers"], d["num_ant_ports"]
        w = np.asarray(d["weights"], np.int16)
        assert w.ndim == 3 and w.shape[0] <= 4 and w.shape[1] <= 8 and w.shape[2] == 2
        full = np.zeros((4, 8, 2), np.int16)
        full[:w.shape[0], :w.shape[1]] = w
        C.memmove(arr[i].weights, full.ctypes.data, full.nbytes)
    return arr, len(mats)


def _pre_args(segs, prgs, pmi_list, pm):
    """the descriptors' PRG records, the flat PMI list and the matrix table as the C calls take them"""
    if len(prgs) != len(segs):
        raise ValueError("one PRG record per descriptor")
    pmi = np.ascontiguousarray(pmi_list if pmi_list is not None else [], np.uint16)
    tab, n_pm = pdsch_pm_table(pm)
    return _struct_array(nrLDPC_hip_pdsch_prg_t, prgs, _PDM_PRG_KEYS), pmi, (pmi.ctypes.data if pmi.size else None), int(pmi.size), tab, n_pm


def pdsch_precode_host(layers, seg, prg, pmi_list, pm, n_tx, ant, tx):
    """nrLDPC_hip_pdsch_precode_host: one descriptor, antenna `ant` of n_tx, on the CPU (csrc/nr_pdsch_map.h, no GPU).  prg = dict with
    prg_size, pmi_off, pmi_count; pmi_list = the flat PMI list; pm = the matrix table (dicts, see pdsch_pm_table) or None.  tx = int16
    grid (written in place at seg's tx_off).  Returns tx."""
    assert layers.dtype == np.int16 and tx.dtype == np.int16 and layers.flags.c_contiguous and tx.flags.c_contiguous
    _pdm_check_extent([seg], 1, 0, layers.size // 2, tx.size // 2)
    garr, keep, pmi_p, n_pmi, tab, n_pm = _pre_args([seg], [prg], pmi_list, pm)
    _check(_pre_lib().nrLDPC_hip_pdsch_precode_host(layers.ctypes.data, _pdm_seg_array([seg]), garr, pmi_p, n_pmi, tab, n_pm, n_tx, ant, tx.ctypes.data),
           "nrLDPC_hip_pdsch_precode_host")
    return tx


def pdsch_precode_segments(allocs, alloc_prgs, n_pmi, cap=None):
    """nrLDPC_hip_pdsch_precode_segments: allocs as for pdsch_map_segments, alloc_prgs = one dict (prg_size, pmi_off, pmi_count) per
    allocation, n_pmi = the length of the flat PMI list.  Returns (descriptors, their PRG records), two lists of dicts."""
    n = len(allocs)
    if len(alloc_prgs) != n:
        raise ValueError("one PRG record per allocation")
    arr, garr = _struct_array(nrLDPC_hip_pdsch_alloc_t, allocs, _PDM_ALLOC_KEYS), _struct_array(nrLDPC_hip_pdsch_prg_t, alloc_prgs, _PDM_PRG_KEYS)
    cap = 14 * n if cap is None else cap
    out, gout, n_out = (nrLDPC_hip_pdsch_map_seg_t * max(cap, 1))(), (nrLDPC_hip_pdsch_prg_t * max(cap, 1))(), C.c_uint32(0)
    _check(_pre_lib().nrLDPC_hip_pdsch_precode_segments(arr, garr, n, n_pmi, out, gout, cap, C.byref(n_out)), "nrLDPC_hip_pdsch_precode_segments")
    return ([{k: (list(out[i].port) if k == "port" else int(getattr(out[i], k))) for k in _PDM_SEG_KEYS} for i in range(n_out.value)],
            [{k: int(getattr(gout[i], k)) for k in _PDM_PRG_KEYS} for i in range(n_out.value)])


def pdsch_resource_mapping_precoded(layers, tx, tx_ant_stride, n_tx, segs, prgs, pmi_list, pm, stream=None):
    """nrLDPC_hip_pdsch_resource_mapping_precoded: as pdsch_resource_mapping plus prgs = one dict (prg_size, pmi_off, pmi_count) per
    descriptor (pdsch_precode_segments), pmi_list = the flat PMI list and pm = the matrix table (dicts, see pdsch_pm_table; None: no
    table) -- host memory in both modes.  numpy int16 arrays -> host call; torch int16 CUDA tensors -> device call enqueued on
    `stream`.  Returns tx."""
    ptr, numel, mem, s = _mem_of((tx, layers), stream)
    _pdm_check_extent(segs, n_tx, tx_ant_stride, numel(layers) // 2, numel(tx) // 2)
    garr, keep, pmi_p, n_pmi, tab, n_pm = _pre_args(segs, prgs, pmi_list, pm)
    _check(_pre_lib().nrLDPC_hip_pdsch_resource_mapping_precoded(ptr(layers), ptr(tx), tx_ant_stride, n_tx, _pdm_seg_array(segs), garr, len(segs), pmi_p,
                                                                 n_pmi, tab, n_pm, mem, s), "nrLDPC_hip_pdsch_resource_mapping_precoded")
    return tx
