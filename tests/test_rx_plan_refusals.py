"""The refusals of the UL receive front's eight entry points (channel_level, channel_compensation, their _grid forms, the two-layer
MMSE and ML receivers and their level calls), HOST mem, on a machine without a GPU: every refusal of csrc/rx_plan.h, of
rxf_check_common / rxm_check_common / check_mem and of the null checks happens before either call scope is opened, so the call
returns without touching a device.  The full text of last_error() is compared: a change to the plans must leave every refusal
byte-identical.  The descriptors are those of the bad_calls tables of test_gpu_rx_front / _grid / _mmse / _ml (fft_size 128, at
most two segments), with the bounds those tables lack.  The three grid descriptors with fft_size 2^21 (nb_re * Qm above 2^21 needs
that many subcarriers to pass the grid checks first) are refused like the others: no array is read."""
import numpy as np
import pytest

FULL, DMRS1, DMRS2 = 0, 1, 2
N, RS, CS = 128, 256, 136

# name -> (the wrapper module's library getter, grid descriptors?, arrays ahead of n_rx, strides, arrays behind n_seg)
CALLS = {
    "channel_compensation": ("_rxf_lib", False, ("rx", "ch"), (64,), ("shift", "rec")),
    "channel_level": ("_rxf_lib", False, ("ch",), (64,), ("out",)),
    "channel_compensation_grid": ("_rxg_lib", True, ("rx", "ch"), (RS, CS), ("shift", "rec")),
    "channel_level_grid": ("_rxg_lib", True, ("ch",), (CS,), ("out",)),
    "mmse_2layers_grid": ("_rxm_lib", True, ("rx", "ch"), (RS, CS), ("shift", "nvar", "rec")),
    "channel_level_grid_mmse": ("_rxm_lib", True, ("ch",), (CS,), ("max_ch", "out")),
    "ml_2layers_grid": ("_rxl_lib", True, ("rx", "ch"), (RS, CS), ("shift", "llr")),
    "channel_level_grid_ml": ("_rxl_lib", True, ("ch",), (CS,), ("max_ch", "out")),
}
RECEIVERS = ("channel_compensation", "channel_compensation_grid", "mmse_2layers_grid", "ml_2layers_grid")
LEVELS = ("channel_level", "channel_level_grid", "channel_level_grid_mmse", "channel_level_grid_ml")
# what a refusal of the plan calls the entry point: the _grid compensation's own checks are the extracted form's
PLAN_NAME = {"channel_compensation": "channel_compensation", "channel_compensation_grid": "channel_compensation",
             "mmse_2layers_grid": "mmse_2layers_grid", "ml_2layers_grid": "ml_2layers_grid"}
PLAIN = dict(tb=0, Qm=4, nb_re=16, plane=32, sym_off=4, rx_off=0, ch_off=0, rec_off=0)
GRID = dict(PLAIN, pattern=DMRS1, fft_size=N, start_re=100, rx_off=N, ch_off=3)
GOOD = {"channel_compensation": PLAIN, "channel_level": PLAIN, "channel_compensation_grid": GRID, "channel_level_grid": GRID,
        "mmse_2layers_grid": dict(GRID, Qm=6, plane=64), "channel_level_grid_mmse": dict(GRID, Qm=6, plane=64),
        "ml_2layers_grid": dict(GRID, plane=64), "channel_level_grid_ml": dict(GRID, plane=64)}
MEM = ": mem must be NRLDPC_HIP_MEM_HOST or NRLDPC_HIP_MEM_DEVICE"
COUNT = ": nb_re above the pattern's count within fft_size subcarriers (p(nb_re - 1) >= fft_size)"
QM = {"channel_compensation": "channel_compensation: Qm must be 2, 4, 6 or 8",
      "channel_compensation_grid": "channel_compensation: Qm must be 2, 4, 6 or 8",
      "mmse_2layers_grid": "mmse_2layers_grid: Qm must be 6 or 8 (two layers of QPSK / 16QAM take the ML receiver, ml_2layers_grid)",
      "ml_2layers_grid": "ml_2layers_grid: Qm must be 2 or 4 (two layers of 64QAM / 256QAM take the MMSE receiver, mmse_2layers_grid)"}
BAD_QM = {"channel_compensation": (5, 0), "channel_compensation_grid": (5, 0), "mmse_2layers_grid": (4, 2, 7), "ml_2layers_grid": (6, 8, 3)}
N_RX = {name: (": n_rx must be 2 or 4", (1, 3, 5, 8)) if name.endswith("mmse") or name.startswith("mmse") else (": n_rx must be 1..8", (0, 9))
        for name in CALLS}


def cases():
    """(id, entry point, segments, keyword arguments of call(), return value, last_error() -- None where the call is accepted)"""
    out = []

    def add(tag, name, segs, want, rc=-1, **kw):
        out.append((f"{name}-{tag}", name, segs, kw, rc, want))

    for name, (_, grid, ahead, _, behind) in CALLS.items():
        good = GOOD[name]
        for arr in ahead + behind:
            add(f"null-{arr}", name, [good], "null argument", **{arr: None})
        add("null-desc", name, [good], "null argument", desc=False)
        text, bad = N_RX[name]
        for n in bad:
            add(f"n_rx{n}", name, [good], name + text, n=n)
        add("mem", name, [good], name + MEM, mem=7)
        add("nothing", name, [], None, rc=0)
        if grid:
            who = "channel_level_grid" if name in LEVELS else name        # the two-layer level calls run the grid's plan
            add("pattern", name, [dict(good, pattern=3)], who + ": pattern must be FULL, DMRS1 or DMRS2")
            add("fft-above", name, [dict(good, fft_size=(1 << 21) + 1)], who + ": fft_size above 2^21")
            add("start_re", name, [dict(good, start_re=N)], who + ": start_re must be below fft_size")
            add("fft0", name, [dict(good, fft_size=0)], who + ": start_re must be below fft_size")
            add("count-dmrs1", name, [dict(good, plane=300, nb_re=65)], who + COUNT)                     # DMRS1: 64 within 128
            add("count-dmrs2", name, [dict(good, plane=300, pattern=DMRS2, nb_re=85)], who + COUNT)      # DMRS2: 84
            add("count-full", name, [dict(good, plane=300, pattern=FULL, nb_re=129)], who + COUNT)
    for name in LEVELS:
        good = GOOD[name]
        who = "channel_level" if name == "channel_level" else "channel_level_grid"   # the two-layer level calls run the grid's plan
        add("no-REs", name, [dict(good, nb_re=0)], who + ": the measurement symbol has no REs")
        add("tb-above", name, [dict(good, tb=1)], who + ": every tb below n_tb must be named once")
        add("tb-twice", name, [good, good], who + ": every tb below n_tb must be named once")
        add("2^20", name, [dict(good, nb_re=(1 << 20) + 1)], who + ": nb_re above 2^20")                # 2 nb_re above 2^21
    for name in RECEIVERS:
        good, who = GOOD[name], PLAN_NAME[name]
        two = name in ("mmse_2layers_grid", "ml_2layers_grid")
        for q in BAD_QM[name]:
            add(f"Qm{q}", name, [dict(good, Qm=q)], QM[name])
        add("odd", name, [dict(good, rec_off=3)], who + ": rec_off must be even")
        add("plane", name, [dict(good, sym_off=17)], who + (": 2 (sym_off + nb_re) above plane" if two else ": sym_off + nb_re above plane"))
        add("empty-segment", name, [dict(good, nb_re=0)], None, rc=0)
        if two:
            add("overlap", name, [dict(good, sym_off=0, nb_re=16), dict(good, sym_off=15, nb_re=8)], who + ": the output ranges of two segments overlap")
        else:
            add("overlap", name, [good, dict(good, sym_off=10, nb_re=8)], who + ": the output ranges of two segments overlap")   # within plane 0
            add("overlap-planes", name, [good, dict(good, Qm=2, rec_off=2 * 32, sym_off=19, nb_re=2)],
                who + ": the output ranges of two segments overlap")                                   # its plane 0 on the other's plane 1
    big = dict(pattern=FULL, fft_size=1 << 21)
    add("2^21", "channel_compensation", [dict(PLAIN, Qm=8, nb_re=(1 << 18) + 1, plane=1 << 19)], "channel_compensation: nb_re * Qm above 2^21")
    add("2^21", "channel_compensation_grid", [dict(GRID, Qm=8, nb_re=(1 << 18) + 1, plane=1 << 19, **big)], "channel_compensation: nb_re * Qm above 2^21")
    add("2^21", "mmse_2layers_grid", [dict(GRID, Qm=8, nb_re=(1 << 17) + 1, plane=1 << 19, **big)], "mmse_2layers_grid: 2 nb_re * Qm above 2^21")
    add("2^21", "ml_2layers_grid", [dict(GRID, nb_re=(1 << 18) + 1, plane=1 << 20, **big)], "ml_2layers_grid: 2 nb_re * Qm above 2^21")
    add("overlap-Qm", "ml_2layers_grid", [dict(GOOD["ml_2layers_grid"], Qm=2, sym_off=0, nb_re=16),
                                          dict(GOOD["ml_2layers_grid"], Qm=4, rec_off=60, sym_off=0, nb_re=4)],
        "ml_2layers_grid: the output ranges of two segments overlap")                                  # int16 60 .. 63 twice
    # n_rx = 3: the MMSE receiver refuses it (above); the ML receiver's plan takes it
    add("n_rx3", "ml_2layers_grid", [dict(GOOD["ml_2layers_grid"], nb_re=0)], None, rc=0, n=3)
    return out


CASES = cases()


def call(m, name, segs, n=2, mem=None, desc=True, **swap):
    """swap: an array's name -> None"""
    lib, grid, ahead, strides, behind = CALLS[name]
    arrays = {k: np.zeros(64, np.int32) for k in ahead + behind}
    ptr = lambda k: None if k in swap else arrays[k].ctypes.data
    seg = (m._rx_grid_seg_array if grid else m._rx_seg_array)(segs) if desc else None
    f = getattr(getattr(m, lib)(), "nrLDPC_hip_ulsch_" + name)
    return f(*[ptr(k) for k in ahead], n, *strides, seg, len(segs), *[ptr(k) for k in behind], m.MEM_HOST if mem is None else mem, None)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_refusal_text(built, case):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    _, name, segs, kw, rc, want = case
    assert call(m, name, segs, **kw) == rc
    if want is not None:
        assert m.last_error() == want
