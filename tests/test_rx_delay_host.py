"""The PUSCH delay search, CPU only: the host form (nrLDPC_hip_pusch_est_delay_host, csrc/nr_delay.h) against the float64 model
(rx_delay_np.py) -- delays equal, peak amplitudes within B(N) --, the kernels of csrc/tb_rx_delay.hip run on the CPU
(tests/emul/slot_delay_emul.cpp) against the host form -- delays and peaks bit for bit --, the stand-alone sanitizer run of the
emulation, the margins of the cases, the misreadings the cases notice and the refusals of the interface.

The cases are fixed and seeded; every result of every case has a margin of at least 8 B(N) (test_every_case_has_its_margin: none
is skipped for lack of it), so fp32 and float64 must agree on it.

Where the largest sample can lie.  x repeats each LS value over four REs (type 1) or six (type 2), so y[n] = R[n] G[n] with G of
period N/4 (N/6) and |R[n]| = |sin(4 pi n / N) / sin(pi n / N)| (six: 6 pi n / N), which falls from n = 0 to a zero at N/4 (N/6)
and is zero at N/2: the largest sample always lies within N/8 (N/12) of 0, y[N/2] is 0 for every grid, and P[N/2 + 1] < P[1].  No
grid puts a peak at N/2 or N/2 + 1.  The peaks are placed at 0, 1, 20, 21, N - 21 and N - 1; the fold at N/2 and N/2 + 1 is
checked on the scan with synthetic spectra (the model) and on nr_dly_fold itself (the emulation's export).

Misreadings (test_the_cases_notice_every_misreading applies each to the model and requires that a delay or a peak of some case
changes):
  exponent_sign     exp(-...) in the transform
  fold_ge           >= instead of > at the N/2 fold (on the synthetic spectra: see above)
  mode_swapped      per antenna where the running maximum is asked, and the reverse
  own_res           the pilots' products at their own REs instead of the pair's value over its group
  t2_drop45         type 2 REs 4, 5 of a block left out
  delta_ignored     delta / nushift of ports 2, 3 ignored
  antennas_swapped  a descriptor's antennas in reverse order
  grid_indexed      x indexed by grid position instead of from the allocation's first RE: a circular shift of x by start_re, which
                    multiplies y[n] by a phase and leaves every P[n] as it is.  No case can notice it; the test asserts that the
                    model's results are unchanged by it, so that nobody looks for a case that would.
"""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rx_chest_np as R
import rx_delay_np as D

ROOT = Path(__file__).resolve().parent.parent
EMUL = ROOT / "tests" / "emul"
CSRC = ROOT / "openairinterface5g_amd" / "csrc"
CLANG = "/opt/rocm/lib/llvm/bin/clang"
CXXFLAGS = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-pass-failed", "-Wno-unused-function", "-I", str(EMUL / "hip_host"), "-I", str(CSRC)]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g"]

T1I, T2I, T1A, T2A = 0, 1, 2, 3
SIZES = (128, 256, 512, 1024, 1536, 2048, 4096, 6144, 8192)
FILL_D, FILL_P = 0x5a5a5a5a, -7.0


# ---------------------------------------------------------------------------------------------------------
# the cases.  A descriptor: dict(mode, port, N, rb, k0, tau per antenna, amp per antenna, zero); each on a symbol of its own.
# The antennas' gains differ (by a fifth from one to the next unless given): a running maximum over equal peaks would have no margin
# ---------------------------------------------------------------------------------------------------------
def _d(mode, port, N, rb, k0, tau, amp=None, zero=False):
    return dict(mode=mode, port=port, N=N, rb=rb, k0=k0, tau=tuple(tau), amp=tuple(amp or [2000.0 * 1.2 ** a for a in range(len(tau))]), zero=zero)


CASES = {
    # all nine sizes in one call, both types in turn, 12 rb about a third of N; two averaging descriptors and an all-zero symbol besides
    "nine-sizes": dict(seed=1, n_rx=2, descs=[_d(i & 1, 0, N, N // 30 + 1, (7 * N // 8) & ~1, (3 + i % 4, -(2 + i % 3))) for i, N in enumerate(SIZES)]
                       + [_d(T1A, 0, 256, 5, 10, (0, 0)), _d(T2A, 1, 512, 7, 20, (0, 0)), _d(T1I, 0, 256, 6, 100, (0, 0), zero=True)]),
    "rb1": dict(seed=2, n_rx=1, descs=[_d(T1I, 0, 128, 1, 20, (2,)), _d(T2I, 0, 128, 1, 30, (-1,))]),
    "rb2": dict(seed=3, n_rx=1, descs=[_d(T1I, 1, 128, 2, 20, (-3,)), _d(T2I, 1, 128, 2, 30, (2,))]),
    "full-1536": dict(seed=4, n_rx=1, descs=[_d(T1I, 0, 1536, 128, 768, (-9,))]),
    "275prb-4096": dict(seed=5, n_rx=1, descs=[_d(T1I, 0, 4096, 275, 398, (11,))]),
    # the peaks' positions: around 0, both sides of the estimator's clamp at 20, and their negatives behind the fold
    "peaks-t1": dict(seed=6, n_rx=1, descs=[_d(T1I, 0, 256, 10, 40, (t,)) for t in (0, 1, 20, 21, -21, -1)]),
    "peaks-t2": dict(seed=7, n_rx=1, descs=[_d(T2I, 0, 512, 20, 40, (t,)) for t in (0, 1, 20, 21, -21, -1)]),
    # three antennas whose peak powers are ordered (mid, high, low) and (high, low, mid), at different positions
    "nrx3-order": dict(seed=8, n_rx=3, descs=[_d(T1I, 0, 256, 8, 16, (3, -5, 9), (2000.0, 3000.0, 1000.0)),
                                              _d(T2I, 1, 512, 12, 16, (-4, 6, 2), (3000.0, 1000.0, 2000.0))]),
    "nrx8": dict(seed=9, n_rx=8, descs=[_d(T1I, 1, 512, 15, 300, (1, -2, 3, -4, 5, -6, 7, -8), tuple(1500.0 + 150.0 * a for a in range(8)))]),
    # ports 0, 1, 2 of type 1 (delta 1 for port 2), ports 2 and 3 of type 2 (nushift 1)
    "ports": dict(seed=10, n_rx=2, descs=[_d(T1I, 0, 256, 8, 30, (4, -2)), _d(T1I, 1, 256, 8, 30, (-3, 5)), _d(T1I, 2, 256, 8, 30, (6, -7)),
                                          _d(T2I, 2, 512, 12, 30, (5, -3)), _d(T2I, 3, 512, 12, 30, (-6, 2))]),
    # an allocation across the grid's wrap
    "wrap": dict(seed=11, n_rx=2, descs=[_d(T1I, 2, 256, 10, 200, (7, -4)), _d(T2I, 3, 512, 16, 422, (-5, 8))]),
}
FLAGS = (D.RUNNING_MAX, D.PER_ANTENNA)
# the cases the misreadings are tried on
MIS_CASES = ("rb1", "peaks-t1", "peaks-t2", "nrx3-order", "ports", "wrap")


def put_paths(rng, rx, s, at, re_offset, tau, amp):
    """the pilots of interpolating descriptor s on the symbol that begins at c16 `at` of every antenna of rx [n_rx, stride, 2]: one
    path of delay tau[a] and gain amp[a] per antenna, with light noise; re_offset = 12 times the allocation's first PRB"""
    N, typ, port, k0 = s["fft_size"], s["mode"] & 1, s["port"], s["start_re"]
    p = np.array(R.pusch_dmrs_rx(s["c_init"], port, s["rb_size"], re_offset, typ), np.float64)
    k = np.arange(len(p))
    sh = (port >> 1) & 1
    re = 6 * (k // 2) + k % 2 if typ else 2 * k + sh                            # from the allocation's first RE
    pos = (k0 + re) % N + (sh if typ else 0)                                    # type 2: the wrap comes before nushift
    for a in range(len(rx)):
        h = amp[a] * np.exp(-2j * np.pi * (re + (sh if typ else 0)) * tau[a] / N)
        v = h * (p[:, 0] - 1j * p[:, 1]) / (23170.0 * np.sqrt(2.0)) + 30.0 * (rng.standard_normal(len(p)) + 1j * rng.standard_normal(len(p)))
        rx[a, at + pos] = np.clip(np.rint(np.stack([v.real, v.imag], -1)), -32768, 32767)


@functools.lru_cache(maxsize=None)
def build(name):
    """the grid and descriptors of a case: rx int16 [n_rx, rx_stride, 2], segs with delay_off = 2 + i (n_rx + 1)"""
    c = CASES[name]
    rng = np.random.default_rng(100 + c["seed"])
    n_rx = c["n_rx"]
    L = sum(d["N"] for d in c["descs"])
    rx_stride = L + 7
    rx = rng.integers(-1500, 1501, (n_rx, rx_stride, 2)).astype(np.int16)      # whatever else is on the grid, the other combs too
    segs, at = [], 0
    for i, d in enumerate(c["descs"]):
        N, typ, port, rb, k0 = d["N"], d["mode"] & 1, d["port"], d["rb"], d["k0"]
        prb0 = 3 + i
        s = dict(mode=d["mode"], port=port, fft_size=N, start_re=k0, rb_size=rb, dmrs_offset=12 * prb0 // (3 if typ else 2),
                 c_init=R.c_init_pusch(3, i % 14, 40 + i, i & 1), rx_off=at, ch_off=0, delay_off=2 + i * (n_rx + 1))
        segs.append(s)
        if d["zero"]:
            rx[:, at:at + N] = 0
        elif not d["mode"] >> 1:
            put_paths(rng, rx, s, at, 12 * prb0, d["tau"], d["amp"])
        at += N
    rx.setflags(write=False)
    return dict(c, rx=rx, rx_stride=rx_stride, segs=segs, n_res=2 + len(segs) * (n_rx + 1))


@functools.lru_cache(maxsize=None)
def modelled(name, flags, mis=()):
    """-> per descriptor (delays, peaks, margins), each per antenna"""
    b = build(name)
    ants = [[(int(r), int(i)) for r, i in b["rx"][a]] for a in range(b["n_rx"])]
    return [D.est_delay(ants, s, flags, frozenset(mis)) for s in b["segs"]]


def host_form(m, b, flags):
    """(delays int32, peaks float32) over the call's result arrays, FILL where nothing belongs"""
    d, p = np.full(b["n_res"], FILL_D, np.int32), np.full(b["n_res"], FILL_P, np.float32)
    for s in b["segs"]:
        dd, pp = m.pusch_est_delay_host(b["rx"].reshape(-1, 2), b["rx_stride"], b["n_rx"], s, flags)
        d[s["delay_off"]:s["delay_off"] + b["n_rx"]], p[s["delay_off"]:s["delay_off"] + b["n_rx"]] = dd, pp
    return d, p


# synthetic spectra for the scan: the largest sample at N/2 and at N/2 + 1, a tie (the first wins), and nothing but zeros
def synthetic(N):
    def one(at, v=9.0):
        P = np.ones(N)
        for n in np.atleast_1d(at):
            P[n] = v
        return P
    return [one(N // 2), one(N // 2 + 1), one((5, N // 2)), one(N - 1), np.zeros(N)]


def test_scan_on_synthetic_spectra():
    for N in SIZES:
        for flags in FLAGS:
            d, p, _ = D.scan(synthetic(N), N, flags)
            want = [N // 2, 1 - N // 2, 5, -1, 0] if flags == D.PER_ANTENNA else [N // 2, N // 2, N // 2, N // 2, N // 2]   # ties keep the earlier
            assert d == want and p == ([9.0, 9.0, 9.0, 9.0, 0.0] if flags == D.PER_ANTENNA else [9.0] * 5), (N, flags)


def test_every_case_has_its_margin():
    """no case is skipped for lack of margin: each has it"""
    for name in CASES:
        b = build(name)
        for flags in FLAGS:
            for s, (delays, peaks, margins) in zip(b["segs"], modelled(name, flags)):
                assert min(margins) >= 8 * D.B(s["fft_size"]), (name, flags, s["fft_size"], margins, D.B(s["fft_size"]))


def test_the_model_finds_the_channels_delays():
    """PER_ANTENNA: tau[a]; RUNNING_MAX: the delay of the strongest antenna so far"""
    for name, c in CASES.items():
        for d, (delays, peaks, _) in zip(c["descs"], modelled(name, D.PER_ANTENNA)):
            assert d["mode"] >> 1 or d["zero"] or tuple(delays) == d["tau"], (name, delays, d["tau"])
            assert (not (d["mode"] >> 1 or d["zero"])) or (delays == [0] * c["n_rx"] and peaks == [0.0] * c["n_rx"])
    (a, _, _), (b, _, _) = modelled("nrx3-order", D.RUNNING_MAX)
    assert a == [3, -5, -5] and b == [-4, -4, -4]


def test_the_cases_notice_every_misreading():
    for mis in D.MISREADINGS:
        if mis == "fold_ge":
            changed = [N for N in SIZES if D.scan(synthetic(N), N, D.PER_ANTENNA, frozenset((mis,)))[0] != D.scan(synthetic(N), N, D.PER_ANTENNA)[0]]
            assert changed == list(SIZES)
            continue
        changed = [(k, f) for k in MIS_CASES for f in FLAGS
                   if [r[:2] for r in modelled(k, f, (mis,))] != [r[:2] for r in modelled(k, f)]]
        if mis == "grid_indexed":                                                # a phase on y: see the module's docstring
            for k in MIS_CASES:
                for (d0, p0, _), (d1, p1, _) in zip(modelled(k, D.PER_ANTENNA), modelled(k, D.PER_ANTENNA, (mis,))):
                    assert d0 == d1 and np.allclose(p0, p1, rtol=1e-9)
            continue
        assert changed, mis


@pytest.mark.parametrize("name", list(CASES))
def test_host_form_against_the_model(built, name):
    import openairinterface5g_amd.ldpc as m
    b = build(name)
    for flags in FLAGS:
        d, p = host_form(m, b, flags)
        for s, (delays, peaks, _) in zip(b["segs"], modelled(name, flags)):
            o, N = s["delay_off"], s["fft_size"]
            assert d[o:o + b["n_rx"]].tolist() == delays, (name, flags, N)
            amp, want = np.sqrt(p[o:o + b["n_rx"]].astype(np.float64)), np.sqrt(np.array(peaks))
            print(name, flags, N, "peak amplitude error / B(N):", (np.abs(amp - want) / np.maximum(want, 1e-300) / D.B(N)).max() if want.max() else 0.0)
            assert (np.abs(amp - want) <= D.B(N) * want).all(), (name, flags, N, amp, want)


# ---------------------------------------------------------------------------------------------------------
# the emulated kernels
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    import openairinterface5g_amd.ldpc as m
    so = tmp_path_factory.mktemp("delay_emul") / "libdelay_emul.so"
    subprocess.run([CLANG + "++", "-O2", "-fPIC", "-shared", *CXXFLAGS, "-o", str(so), str(EMUL / "slot_delay_emul.cpp"), "-lpthread"], check=True)
    L = C.CDLL(str(so))
    L.slot_delay_emul_last_error.restype = C.c_char_p
    L.slot_emul_pusch_est_delay.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(m.nrLDPC_hip_chest_seg_t), C.c_uint32, C.c_uint32, C.c_void_p,
                                            C.c_void_p]
    L.slot_emul_delay_fold.argtypes = [C.c_uint32, C.c_uint32]
    L.slot_emul_delay_fold.restype = C.c_int32
    return L


def test_the_fold(built, emul):
    for N in SIZES:
        assert [emul.slot_emul_delay_fold(N, n) for n in (0, 1, N // 2 - 1, N // 2, N // 2 + 1, N - 1)] == [0, 1, N // 2 - 1, N // 2, 1 - N // 2, -1]


# N = 128, 1536 and 8192 are among them ("rb1", "full-1536", "nine-sizes")
@pytest.mark.parametrize("name", list(CASES))
def test_emulated_kernels_equal_the_host_form(built, emul, name):
    import openairinterface5g_amd.ldpc as m
    b = build(name)
    for flags in FLAGS:
        want_d, want_p = host_form(m, b, flags)
        d, p = np.full(b["n_res"], FILL_D, np.int32), np.full(b["n_res"], FILL_P, np.float32)
        for rep in range(2 if name == "ports" else 1):                       # once the same call twice on one set of arrays
            rc = emul.slot_emul_pusch_est_delay(b["rx"].ctypes.data, b["rx_stride"], b["n_rx"], m._chest_seg_array(b["segs"]), len(b["segs"]), flags,
                                                d.ctypes.data, p.ctypes.data)
            assert rc == 0, emul.slot_delay_emul_last_error()
            assert np.array_equal(d, want_d) and np.array_equal(p.view(np.uint32), want_p.view(np.uint32)), (name, flags, rep)   # and nothing but the write set
    if name == "ports":                                                      # without peak
        d = np.full(b["n_res"], FILL_D, np.int32)
        assert emul.slot_emul_pusch_est_delay(b["rx"].ctypes.data, b["rx_stride"], b["n_rx"], m._chest_seg_array(b["segs"]), len(b["segs"]), 0, d.ctypes.data, None) == 0
        assert np.array_equal(d, host_form(m, b, 0)[0])


# ---------------------------------------------------------------------------------------------------------
# refusals (they come before anything is enqueued or written, so HOST mem shows them without a GPU)
# ---------------------------------------------------------------------------------------------------------
def test_refusals(built):
    import openairinterface5g_amd.ldpc as m
    b = build("ports")
    rx = b["rx"].reshape(-1, 2)

    def call(segs=b["segs"], n_rx=b["n_rx"], flags=0):
        m.pusch_est_delay(rx, b["rx_stride"], n_rx, segs, flags)
    with pytest.raises(RuntimeError, match="flags must be"):
        call(flags=2)
    with pytest.raises(RuntimeError, match="delay ranges of two descriptors overlap"):
        call(segs=[b["segs"][0], dict(b["segs"][1], delay_off=b["segs"][0]["delay_off"] + 1)] + b["segs"][2:])
    with pytest.raises(RuntimeError, match="n_rx must be 1..8"):
        call(n_rx=0)
    with pytest.raises(RuntimeError, match="mode must be"):
        call(segs=[dict(b["segs"][0], mode=4)])
    with pytest.raises(RuntimeError, match="rb_size is 0"):
        call(segs=[dict(b["segs"][0], rb_size=0)])
    with pytest.raises(RuntimeError, match="fft_size must be"):
        call(segs=[dict(b["segs"][0], fft_size=768, rb_size=4)])
    with pytest.raises(RuntimeError, match="would be read at index fft_size"):
        call(segs=[dict(b["segs"][3], start_re=511 - 6)])
    L = m._delay_lib()
    segs = m._chest_seg_array(b["segs"])
    d, p = np.full(b["n_res"], FILL_D, np.int32), np.full(b["n_res"], FILL_P, np.float32)
    args = [rx.ctypes.data, b["rx_stride"], b["n_rx"], segs, len(b["segs"]), 0, d.ctypes.data, p.ctypes.data, m.MEM_HOST, None]
    for k in (0, 3, 6):
        a = list(args)
        a[k] = None
        assert L.nrLDPC_hip_pusch_est_delay(*a) != 0 and "null argument" in m.last_error(), k
    assert L.nrLDPC_hip_pusch_est_delay(*args[:8], 7, None) != 0 and "mem must be" in m.last_error()
    for k in (0, 3, 5):
        a = [rx.ctypes.data, b["rx_stride"], b["n_rx"], segs, 0, d.ctypes.data, p.ctypes.data]
        a[k] = None
        assert L.nrLDPC_hip_pusch_est_delay_host(*a) != 0 and "null argument" in m.last_error(), k
    assert L.nrLDPC_hip_pusch_est_delay_host(rx.ctypes.data, b["rx_stride"], b["n_rx"], segs, 3, d.ctypes.data, p.ctypes.data) != 0 and "flags must be" in m.last_error()
    assert (d == FILL_D).all() and (p == FILL_P).all()                       # nothing was written
    # averaging descriptors alone need no GPU in HOST mem: 0 and 0
    avg = [dict(b["segs"][0], mode=T1A), dict(b["segs"][1], mode=T1A)]
    dd, pp = m.pusch_est_delay(rx, b["rx_stride"], b["n_rx"], avg, 1)
    for s in avg:
        assert not dd[s["delay_off"]:s["delay_off"] + 2].any() and not pp[s["delay_off"]:s["delay_off"] + 2].any()


# ---------------------------------------------------------------------------------------------------------
# the interpolating slots of ul_slot_np.py: the search finds the channel's delays, so the estimates are those the slots' tests know
# ---------------------------------------------------------------------------------------------------------
SLOTS = ("1L-T1I-p0", "1L-T2I-p1", "1L-T1I-p2", "2L-T1I", "2L-T2I", "2L-T1I-ml16", "2L-T1I-ml4")


@pytest.mark.parametrize("name", SLOTS)
def test_the_slots_delays_are_found(built, name):
    import openairinterface5g_amd.ldpc as m
    import ul_slot_np as U
    sl = U.slot_of(m, name)
    rx = np.ascontiguousarray(sl["rx"].reshape(-1, 2))
    got = np.zeros_like(sl["delay"])
    for s in sl["csegs"]:
        got[s["delay_off"]:s["delay_off"] + sl["case"]["n_rx"]] = m.pusch_est_delay_host(rx, sl["rx_stride"], sl["case"]["n_rx"], s, D.PER_ANTENNA)[0]
    assert np.array_equal(got, sl["delay"]), (name, got, sl["delay"])


# ---------------------------------------------------------------------------------------------------------
# the emulated kernels under the host sanitizers, on arrays of exactly the documented extents
# ---------------------------------------------------------------------------------------------------------
def test_emulated_kernels_on_exact_buffers_under_the_host_sanitizers(tmp_path):
    """a stand-alone program (its own main): sanitized code is never loaded into Python.  DESIGN.md 4.15"""
    jobs = [subprocess.Popen([CLANG, *SAN, "-c", str(CSRC / "nr_coding_host.c"), "-o", str(tmp_path / "nr_coding_host.o")]),
            subprocess.Popen([CLANG + "++", *SAN, *CXXFLAGS, "-DDELAY_EMUL_MAIN", "-c", str(EMUL / "slot_delay_emul.cpp"), "-o",
                              str(tmp_path / "slot_delay_emul.o")])]
    assert [j.wait() for j in jobs] == [0, 0]
    exe = tmp_path / "delay_emul_san"
    subprocess.run([CLANG + "++", *SAN, "-o", str(exe), str(tmp_path / "nr_coding_host.o"), str(tmp_path / "slot_delay_emul.o"), "-lpthread"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-4000:]
    calls, bad = (int(x) for x in r.stdout.split())
    assert calls == 8 and bad == 0, r.stdout
