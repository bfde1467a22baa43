"""Seeded random draws of the slot-level calls that take descriptor tables, for test_slot_sweep_host.py (the kernels on the CPU) and
test_gpu_slot_sweep.py (the same draws on the GPU).  draw(call, seed) is deterministic from np.random.default_rng([call index,
seed]) and returns everything the call takes: descriptors, input arrays, strides, and the sizes of its output arrays.  Every draw is
valid by construction -- output ranges are laid out one after another with drawn gaps and the descriptors shuffled afterwards; the
library's refusal rules (the nushift rule nr_che_reaches_n, sym_off + nb_re <= plane, even rec_off, nb_re within the pattern's
count, disjoint write sets) are known here and avoided -- so a refusal is a failure of the test that sees it.

Each value is drawn either uniformly or from a short list of seam values with about equal chance (pick); d["seams"] names the
categories a draw hit, SEAMS[call] lists every category of a call (the host test requires each at least three times).

An output array has MARGIN canary elements in front of and behind what the call may write; expected(m, d) gives the whole arrays as
the host forms (the *_host calls of the library, element by element) leave them, run(m, d, ins, outs) makes the library call on
numpy arrays (HOST mem) or torch tensors (DEVICE mem), modelled(m, d) the numpy restatements' result for the draws below a size bound (d["small"]).

A draw kind covers a compensation call together with its level call: "front" is ulsch_channel_level + ulsch_channel_compensation,
"grid", "mmse" and "ml" the same pairs from the OFDM grid."""
import numpy as np

import rx_chest_meas_np as M
import rx_chest_np as R
import rx_delay_np as D
import test_gpu_rx_chest as GCH
import test_gpu_rx_chest_meas as GCM
import test_rx_delay_host as H

CALLS = ("front", "grid", "mmse", "ml", "chest", "chest_meas", "time_avg", "delay", "pdsch_map", "pdsch_precoded")
CANARY = 0x5a5a
FILL32 = 0x5a5a5a5a
MARGIN = 64                              # canary elements (c16, int32 or float32) on either side of every output array
SIZES = (128, 256, 512, 1024, 1536, 2048, 4096, 6144, 8192)
RE_BUDGET = 40000
T1I, T2I, T1A, T2A = 0, 1, 2, 3
RB_SEAMS = (1, 2, 3, 21, 22, 42, 43, 64, 65, 85, 86, 256, 257)
DELAY_SEAMS = (-24, -21, -20, -19, 0, 19, 20, 21, 24)
SEAMS = {}


def pick(rng, seams, lo, hi):
    """a seam value or a uniform one from lo .. hi, with equal chance; -> (value, it came from the list)"""
    seams = [s for s in seams if lo <= s <= hi]
    if seams and rng.random() < 0.5:
        return int(seams[int(rng.integers(0, len(seams)))]), True
    return int(rng.integers(lo, hi + 1)), False


def draw_fft(rng, seams):
    """all nine sizes, 4096 and above in about one draw of four"""
    N = int(rng.choice(SIZES[6:])) if rng.random() < 0.25 else int(rng.choice(SIZES[:6]))
    seams.add(f"fft{N}")
    return N


def full_scale(rng, shape, hot=0.2):
    """int16 values over the whole range, a fifth of them at 32767 / -32768"""
    a = rng.integers(-32768, 32768, shape).astype(np.int16)
    mask = rng.random(shape) < hot
    a[mask] = rng.choice(np.array([32767, -32768], np.int16), int(mask.sum()))
    return a


def lay_out(rng, sizes, first, max_gap):
    """ranges of `sizes` one after another from `first` on with gaps of 0 .. max_gap, assigned to the entries in a drawn order:
    -> (offsets, end).  The entries' own order is then not the order in memory."""
    offs, at = [0] * len(sizes), first
    for i in rng.permutation(len(sizes)):
        offs[int(i)] = at
        at += sizes[int(i)] + int(rng.integers(0, max_gap + 1))
    return offs, at


def with_margin(n, dtype, width=1, fill=CANARY):
    """a canary-filled array of MARGIN + n + MARGIN elements of `width` values each, 16-byte aligned"""
    size = (2 * MARGIN + n) * width
    raw = np.empty(size * np.dtype(dtype).itemsize + 16, np.uint8)
    a = raw[(-raw.ctypes.data) % 16:][:size * np.dtype(dtype).itemsize].view(dtype)
    a[:] = np.array(fill).astype(dtype) if np.dtype(dtype).kind != "f" else fill
    return a


def inner(a, width=1):
    """the part of a with_margin array that the call is given"""
    return a[MARGIN * width:]


# ---------------------------------------------------------------------------------------------------------
# PUSCH channel estimation, its measuring form, the time average and the delay search
# ---------------------------------------------------------------------------------------------------------
def reaches_n(mode, port, N, k0, rb):
    """nr_che_reaches_n of csrc/nr_chest.h: a pilot RE at subcarrier N - 1 that nushift moves to index N"""
    if mode == T1I or not (port >> 1) & 1:
        return False
    used = (lambda t: t % 6 < 2) if mode & 1 else (lambda t: t % 2 == 0)
    return any(used(t) and (k0 + t) % N == N - 1 for t in range(12 * rb))


SEAMS["chest"] = ([f"mode{k}" for k in range(4)] + [f"fft{N}" for N in SIZES] + [f"rb{r}" for r in RB_SEAMS] + ["rb_widest"]
                  + ["start0", "startN-1", "startN-2", "start_wrap", "two_pieces", "nushift", "gold_straddle", "delay_below", "delay_above", "delay_none",
                     "odd_stride", "even_stride", "mixed_fft", "hot_grid"] + [f"ch_res{k}" for k in range(4)]
                  + [f"mode{k}_port{p}" for k in range(4) for p in range(12 if k & 1 else 8)])
SEAMS["chest_meas"] = SEAMS["chest"] + ["several_per_block", "block_without_descriptor"]


def draw_chest_segs(rng, seams, max_seg=8, budget=RE_BUDGET):
    """-> (n_rx, N of the widest, descriptors without ch_off / delay_off / rx_off)"""
    N0 = draw_fft(rng, seams)
    n_rx = min(int(rng.integers(1, 9)), max(1, budget // N0))
    mixed = N0 <= 2048 and rng.random() < 0.3
    left, segs, modes = budget // n_rx, [], (T1I, T2I, T1A, T2A)
    for i in range(int(rng.integers(1, max_seg + 1))):
        N = int(rng.choice([s for s in SIZES if s <= N0])) if mixed and i else N0
        if mixed and N != N0:
            seams.update(("mixed_fft", f"fft{N}"))
        # 256 and 257 PRBs fit the three widest carriers only, so they are drawn more often there
        rb = pick(rng, RB_SEAMS + (N // 12,) + ((256, 257) * 3 if N >= 4096 else ()), 1, N // 12)[0]
        rb = min(rb, left // 12)
        if rb == 0:
            break
        left -= 12 * rb
        mode = int(rng.choice(modes))
        port = int(rng.integers(0, 12 if mode & 1 else 8))
        k0 = pick(rng, [0, N - 1, N - 2] + [(N - 6 * rb + j) % N for j in range(-2, 3)], 0, N - 1)[0]
        for _ in range(8):                                             # the nushift rule: move the allocation, then give the port up
            if not reaches_n(mode, port, N, k0, rb):
                break
            k0 = (k0 + 1) % N
        if reaches_n(mode, port, N, k0, rb):
            port &= ~2
        off = pick(rng, (0, 1, 7, 8, 15, 16, 1900), 0, 1900)[0]
        segs.append(dict(mode=mode, port=port, fft_size=N, start_re=k0, rb_size=rb, dmrs_offset=off, c_init=int(rng.integers(0, 1 << 31))))
        seams.update((f"mode{mode}", f"mode{mode}_port{port}"))
        if rb in RB_SEAMS:
            seams.add(f"rb{rb}")
        if rb == N // 12:
            seams.add("rb_widest")
        seams.update(s for s, hit in (("start0", k0 == 0), ("startN-1", k0 == N - 1), ("startN-2", k0 == N - 2), ("start_wrap", k0 + 12 * rb > N),
                                      ("two_pieces", (rb if mode >> 1 else 3 * rb) > 256), ("nushift", bool(port & 2)),
                                      ("gold_straddle", (2 * off) % 32 > 12)) if hit)
    return n_rx, N0, segs


def draw_chest(rng, seams, meas=False):
    # the measuring kernels have barriers, so their emulation runs every workgroup on 256 real threads: fewer workgroups per draw
    n_rx, N0, segs = draw_chest_segs(rng, seams, 6, 12000) if meas else draw_chest_segs(rng, seams)
    n_sym = int(rng.integers(1, 1 + max(1, min(3, RE_BUDGET // (N0 * n_rx)))))
    n = len(segs)
    ch_off, at = lay_out(rng, [12 * s["rb_size"] for s in segs], int(rng.integers(0, 4)), 5)
    cs = at + int(rng.integers(0, 4))
    dl_off, n_dl = lay_out(rng, [n_rx] * n, int(rng.integers(0, 3)), 2)
    for s, c, o in zip(segs, ch_off, dl_off):
        s.update(ch_off=c, delay_off=o, rx_off=int(rng.integers(0, n_sym)) * N0 + int(rng.integers(0, 4)))
        seams.add(f"ch_res{c % 4}")
    seams.add("odd_stride" if cs & 1 else "even_stride")
    rs = n_sym * N0 + 4 + int(rng.integers(0, 4))
    hot = rng.random() < 0.5
    rx = full_scale(rng, (n_rx * rs, 2), 0.2 if hot else 0.0)
    if hot:
        seams.add("hot_grid")
    delay = None
    if rng.random() < 0.85:
        delay = np.array([pick(rng, DELAY_SEAMS, -24, 24)[0] for _ in range(n_dl)], np.int32)
        used = np.concatenate([delay[s["delay_off"]:s["delay_off"] + n_rx] for s in segs])
        seams.update(s for s, hit in (("delay_below", (used < -20).any()), ("delay_above", (used > 20).any())) if hit)
    else:
        seams.add("delay_none")
    d = dict(n_rx=n_rx, segs=segs, rs=rs, cs=cs, inputs=dict(rx=rx, delay=delay), outputs=dict(ch=(n_rx * cs, np.int16, 2, CANARY)))
    if meas:
        # blocks of (nr_of_symbols, layers); every descriptor names a block, one block may stay without any
        n_tb = int(rng.integers(1, 4))
        blocks = [(int(rng.integers(1, 15)), int(rng.integers(1, 3))) for _ in range(n_tb)]
        seg_tb = [int(rng.integers(0, n_tb)) for _ in segs]
        if n_tb > 1 and rng.random() < 0.3:
            seg_tb = [t if t else 1 for t in seg_tb]
        d.update(seg_tb=seg_tb, blocks=blocks, nvar_div=[s * l * n_rx for s, l in blocks])
        d["outputs"].update(max_ch=(n_tb, np.int32, 1, FILL32), nvar=(n_tb, np.int32, 1, FILL32))
        seams.update(s for s, hit in (("several_per_block", max(seg_tb.count(t) for t in range(n_tb)) > 1),
                                      ("block_without_descriptor", len(set(seg_tb)) < n_tb)) if hit)
    d["small"] = N0 <= (512 if meas else 1536) and n_rx * sum(12 * s["rb_size"] for s in segs) <= (600 if meas else 1200)
    return d


def chest_order(rng, d):
    """the descriptors shuffled (with what runs parallel to them)"""
    order = [int(i) for i in rng.permutation(len(d["segs"]))]
    d["segs"] = [d["segs"][i] for i in order]
    if "seg_tb" in d:
        d["seg_tb"] = [d["seg_tb"][i] for i in order]
    return d


def chest_expected(m, d):
    rx, dl = d["inputs"]["rx"], d["inputs"]["delay"]
    out = {"ch": embed(GCH.host_form(m, d["segs"], rx, d["rs"], d["cs"], d["n_rx"], dl), 2)}
    if "seg_tb" in d:
        mx, nv = GCM.host_form(m, dict(d, rx=rx, rx_stride=d["rs"], est_delay=dl))
        out["max_ch"] = embed(np.array(mx, np.int32), 1, FILL32)
        out["nvar"] = embed(np.array(nv, np.uint32).view(np.int32), 1, FILL32)
    return out


def embed(a, width, fill=CANARY):
    """`a` between two margins of canaries, flat"""
    a = np.ascontiguousarray(a).reshape(-1)
    out = np.empty(a.size + 2 * MARGIN * width, a.dtype)
    out[:] = np.array(fill).astype(a.dtype)
    out[MARGIN * width:MARGIN * width + a.size] = a
    return out


def chest_run(m, d, ins, outs):
    if "seg_tb" in d:
        res = m.pusch_channel_estimation_meas(ins["rx"], d["rs"], outs["ch"], d["cs"], d["n_rx"], d["segs"], d["seg_tb"], d["nvar_div"], ins["delay"],
                                              outs["max_ch"], outs["nvar"])
        if isinstance(ins["rx"], np.ndarray):                           # HOST mem returns the two
            n = len(d["nvar_div"])
            outs["max_ch"][:n], outs["nvar"][:n] = res[1], res[2].view(np.int32)
    else:
        m.pusch_channel_estimation(ins["rx"], d["rs"], outs["ch"], d["cs"], d["n_rx"], d["segs"], ins["delay"])


def chest_modelled(m, d):
    """rx_chest_np.py per (descriptor, antenna), rx_chest_meas_np.py per block"""
    rx, dl, n_rx = d["inputs"]["rx"], d["inputs"]["delay"], d["n_rx"]
    ch = np.full((n_rx * d["cs"], 2), CANARY, np.int16)
    ants = [[(int(r), int(i)) for r, i in rx[a * d["rs"]:(a + 1) * d["rs"]]] for a in range(n_rx)]
    calls = []
    for s in d["segs"]:
        dls = [int(dl[s["delay_off"] + a]) if dl is not None else 0 for a in range(n_rx)]
        re_offset = s["dmrs_offset"] * (3 if s["mode"] & 1 else 2)       # nr_dmrs_rx.c:84 back
        calls.append(dict(rx_ants=ants, soffset=s["rx_off"], N=s["fft_size"], k0=s["start_re"], nb_rb=s["rb_size"], p=s["port"], dmrs_type=s["mode"] & 1,
                          chest_freq=s["mode"] >> 1, c_init=s["c_init"], re_offset=re_offset, est_delays=dls, layer=0))
        for a in range(n_rx):
            est = R.pusch_channel_estimation(ants[a], s["rx_off"], s["fft_size"], s["start_re"], s["rb_size"], s["port"], s["mode"] & 1, s["mode"] >> 1,
                                             s["c_init"], re_offset, dls[a], literal_type2_avg=False)
            o = s["ch_off"] + a * d["cs"]
            ch[o:o + 12 * s["rb_size"]] = np.array(est[:12 * s["rb_size"]], np.int64).astype(np.int16)
    out = {"ch": embed(ch, 2)}
    if "seg_tb" in d:
        mx, nv = [], []
        for tb, (n_symbols, layers) in enumerate(d["blocks"]):
            r = M.pdu_measurements([c for c, t in zip(calls, d["seg_tb"]) if t == tb], n_symbols, layers, n_rx)
            mx.append(r[0])
            nv.append(r[1])
        out["max_ch"] = embed(np.array(mx, np.int32), 1, FILL32)
        out["nvar"] = embed(np.array(nv, np.uint32).view(np.int32), 1, FILL32)
    return out


# ---- the time average -------------------------------------------------------------------------------------------------------
SEAMS["time_avg"] = [f"n_sym{k}" for k in (2, 3, 4)] + [f"planes{k}" for k in range(1, 9)] + [f"rb{r}" for r in RB_SEAMS] + ["second_piece", "saturates"]


def draw_time_avg(rng, seams):
    n_plane = int(rng.integers(1, 9))
    seams.add(f"planes{n_plane}")
    left, sizes, segs = RE_BUDGET // n_plane, [], []
    for _ in range(int(rng.integers(1, 9))):
        n_sym = int(rng.integers(2, 5))
        rb = min(pick(rng, RB_SEAMS, 1, 300)[0], left // (12 * n_sym))
        if rb == 0:
            break
        left -= 12 * rb * n_sym
        segs.append(dict(n_sym=n_sym, rb_size=rb))
        sizes += [12 * rb] * n_sym
        seams.add(f"n_sym{n_sym}")
        if rb in RB_SEAMS:
            seams.add(f"rb{rb}")
        if rb > 256:
            seams.add("second_piece")
    offs, at = lay_out(rng, sizes, int(rng.integers(0, 4)), 5)              # every symbol of every descriptor a range of its own
    for s in segs:
        s["ch_off"], offs = offs[:s["n_sym"]], offs[s["n_sym"]:]
    stride = at + int(rng.integers(0, 4))
    hot = rng.random() < 0.5
    ch = full_scale(rng, ((n_plane - 1) * stride + at, 2), 0.2 if hot else 0.0)
    if not hot:
        ch >>= int(rng.integers(0, 3))
    else:
        seams.add("saturates")
    return dict(n_plane=n_plane, stride=stride, segs=segs, inputs={}, outputs=dict(ch=(len(ch), np.int16, 2, CANARY)), init=dict(ch=ch),
                small=n_plane * sum(sizes) <= 12000)


def time_avg_expected(m, d):
    ch = d["init"]["ch"].copy()
    for s in d["segs"]:
        for q in range(d["n_plane"]):
            m.pusch_chest_time_avg_host(ch, dict(s, ch_off=[o + q * d["stride"] for o in s["ch_off"]]))
    return {"ch": embed(ch, 2)}


def time_avg_run(m, d, ins, outs):
    m.pusch_chest_time_avg(outs["ch"], d["stride"], d["n_plane"], d["segs"])


def time_avg_modelled(m, d):
    ch = d["init"]["ch"]
    out = ch.copy()
    for s in d["segs"]:
        for q in range(d["n_plane"]):
            syms = [[(int(r), int(i)) for r, i in ch[o + q * d["stride"]:o + q * d["stride"] + 12 * s["rb_size"]]] for o in s["ch_off"]]
            o = s["ch_off"][0] + q * d["stride"]
            out[o:o + 12 * s["rb_size"]] = np.array(M.chest_time_domain_avg(syms), np.int64).astype(np.int16)
    return {"ch": embed(out, 2)}


# ---- the delay search -------------------------------------------------------------------------------------------------------
# both kinds cover both flags, with and without `peak`, and mix averaging descriptors: those seams are counted per kind
SEAMS["delay"] = (["kind_a", "kind_b", "equal_antennas", "tie_running_max", "amp3", "amp200", "amp_full", "type1", "type2", "small_fft", "big_fft"]
                  + [f"{k}_{x}" for k in "ab" for x in ("flags0", "flags1", "with_peak", "without_peak", "averaging_mixed")])
DELAY_BUDGET = 12000                     # c16 of grid per draw: the emulated search takes 0.2 - 0.4 s at twice that


def draw_delay(rng, seams):
    """kind (a): arbitrary grids, in a third of them every antenna the same; kind (b): one path per antenna as
    test_rx_delay_host.build makes them"""
    kind_b = rng.random() < 0.5
    k = "b" if kind_b else "a"
    seams.add(f"kind_{k}")
    equal = not kind_b and rng.random() < 1 / 3                        # kind (a): every antenna the same grid
    N0 = draw_fft(rng, set())                                          # (the sizes themselves are no seam of this kind: big or small is)
    seams.add("big_fft" if N0 >= 4096 else "small_fft")
    n_rx = min(int(rng.integers(1, 9)), max(2, DELAY_BUDGET // (2 * N0)))
    n_seg = int(rng.integers(1, 1 + max(1, min(8, DELAY_BUDGET // (N0 * n_rx)))))
    segs, taus = [], []
    for i in range(n_seg):
        N = N0 if i == 0 or rng.random() < 0.5 else int(rng.choice([s for s in SIZES if s <= N0]))
        mode = int(rng.integers(0, 2))
        if i and rng.random() < 0.2:
            mode += 2
            seams.add(f"{k}_averaging_mixed")
        seams.add("type2" if mode & 1 else "type1")
        port = int(rng.integers(0, 4))
        # kind (b): an allocation of at least a sixth of the carrier, so that the peak's neighbours lie 8 B(N) below it
        rb = int(rng.integers(max(1, N // 72 + 1), N // 12 + 1)) if kind_b else pick(rng, (1, 2, 3, 22, 86, N // 12), 1, N // 12)[0]
        k0 = pick(rng, (0, N - 2, (N - 6 * rb) % N), 0, N - 1)[0]
        for _ in range(8):
            if not reaches_n(mode, port, N, k0, rb):
                break
            k0 = (k0 + 1) % N
        if reaches_n(mode, port, N, k0, rb):
            port &= ~2
        segs.append(dict(mode=mode, port=port, fft_size=N, start_re=k0, rb_size=rb, dmrs_offset=int(rng.integers(0, 1901)),
                         c_init=int(rng.integers(0, 1 << 31)), rx_off=i * N0 + int(rng.integers(0, 3)), ch_off=0))
        # x repeats an LS value over four REs (six for type 2), so a path at tau has an image N/4 (N/6) away that is as strong at
        # |tau| = N/8 (N/12): the delays stay well inside that
        lim = min(24, N // 20 if mode & 1 else N // 12)
        taus.append([pick(rng, (0, 1, 20, 21, -21, -1), -lim, lim)[0] for _ in range(n_rx)])
    rs = n_seg * N0 + 3 + int(rng.integers(0, 4))
    if kind_b:
        rx = rng.integers(-1500, 1501, (n_rx, rs, 2)).astype(np.int16)
        gains = 2000.0 * 1.2 ** rng.permutation(n_rx)                    # a fifth apart, in a drawn order
        for s, tau in zip(segs, taus):
            if not s["mode"] >> 1:
                H.put_paths(rng, rx, s, s["rx_off"], s["dmrs_offset"] * (3 if s["mode"] & 1 else 2), tau, gains)
    else:
        amp = int(rng.choice([3, 200, 32768], p=[0.4, 0.3, 0.3]))          # the smallest grids have the most ties
        seams.add({3: "amp3", 200: "amp200", 32768: "amp_full"}[amp])
        rx = rng.integers(-amp, amp, (n_rx, rs, 2)).astype(np.int16)
        if equal:
            rx[:] = rx[0]
            seams.add("equal_antennas")
    offs, n_res = lay_out(rng, [n_rx] * n_seg, int(rng.integers(0, 3)), 2)
    for s, o in zip(segs, offs):
        s["delay_off"] = o
    flags, peak = int(rng.integers(0, 2)), bool(rng.integers(0, 2))
    if equal and rng.random() < 0.5:                    # equal antennas meet the running maximum more often than not
        flags = 0
    seams.update((f"{k}_flags{flags}", f"{k}_with_peak" if peak else f"{k}_without_peak"))
    if equal and flags == 0 and n_rx > 1:               # a later antenna's peak is exactly the earlier one's
        seams.add("tie_running_max")
    outputs = dict(est_delay=(n_res, np.int32, 1, FILL32))
    if peak:
        outputs["peak"] = (n_res, np.float32, 1, -7.0)
    return dict(n_rx=n_rx, segs=segs, rs=rs, flags=flags, kind_b=kind_b, inputs=dict(rx=rx.reshape(-1, 2)), outputs=outputs, small=kind_b)


def delay_expected(m, d):
    n_res, n_rx = d["outputs"]["est_delay"][0], d["n_rx"]
    dl, pk = np.full(n_res, FILL32, np.int32), np.full(n_res, -7.0, np.float32)
    for s in d["segs"]:
        dl[s["delay_off"]:s["delay_off"] + n_rx], pk[s["delay_off"]:s["delay_off"] + n_rx] = m.pusch_est_delay_host(d["inputs"]["rx"], d["rs"], n_rx, s, d["flags"])
    out = {"est_delay": embed(dl, 1, FILL32)}
    if "peak" in d["outputs"]:
        out["peak"] = embed(pk, 1, -7.0)
    return out


def delay_run(m, d, ins, outs):
    res = m.pusch_est_delay(ins["rx"], d["rs"], d["n_rx"], d["segs"], d["flags"], outs["est_delay"], outs.get("peak"))
    if isinstance(ins["rx"], np.ndarray):                               # HOST mem returns arrays of its own: only the write set is defined
        for s in d["segs"]:
            o = slice(s["delay_off"], s["delay_off"] + d["n_rx"])
            outs["est_delay"][o] = res[0][o]
            if "peak" in outs:
                outs["peak"][o] = res[1][o]


def delay_modelled(m, d):
    """kind (b): -> per descriptor (delays, peaks, margins) of rx_delay_np.py"""
    rx = d["inputs"]["rx"].reshape(d["n_rx"], d["rs"], 2)
    ants = [[(int(r), int(i)) for r, i in rx[a]] for a in range(d["n_rx"])]
    return [D.est_delay(ants, s, d["flags"]) for s in d["segs"]]


# ---------------------------------------------------------------------------------------------------------
# The receive front: extracted arrays ("front"), the OFDM grid ("grid"), the two-layer MMSE and ML receivers ("mmse", "ml")
# ---------------------------------------------------------------------------------------------------------
FULL, DMRS1, DMRS2 = 0, 1, 2
NB_SEAMS = (0,) + tuple(range(1, 8)) + tuple(range(1020, 1029)) + tuple(range(2044, 2053))
SHIFT_SEAMS = {"front": (0, 1, 7, 12, 15, 16, 31), "grid": (0, 1, 7, 12, 15, 16, 31), "mmse": (0, 3, 6, 9), "ml": (0, 3, 6, 9)}
RX_QM = {"front": (2, 4, 6, 8), "grid": (2, 4, 6, 8), "mmse": (6, 8), "ml": (2, 4)}
_rx_common = (["nb0", "nb1-7", "nb1020-1028", "nb2044-2052", "two_workgroups", "three_workgroups"] + [f"sym_res{k}" for k in range(4)]
              + [f"ch_res{k}" for k in range(4)] + ["odd_stride", "even_stride", "blocks2", "blocks3", "moderate_channel"])
SEAMS["front"] = _rx_common + [f"Qm{q}" for q in RX_QM["front"]] + [f"n_rx{k}" for k in range(1, 9)] + [f"phase{k}" for k in range(4)] + ["phase_adds_workgroup"]
_grid = [f"pattern{k}" for k in range(3)] + [f"fft{N}" for N in SIZES] + [f"wrap_in_group{k}" for k in range(4)] + ["no_wrap", "start0"]
SEAMS["grid"] = SEAMS["front"] + _grid
SEAMS["mmse"] = _rx_common + _grid + ["Qm6", "Qm8", "n_rx2", "n_rx4", "nvar0", "nvar_set", "max_ch_scaled", "max_ch_plain"]
SEAMS["ml"] = _rx_common + _grid + ["Qm2", "Qm4", "max_ch_scaled", "max_ch_plain"] + [f"n_rx{k}" for k in range(1, 9)]


def rxg_p(pattern, j):
    """the PUSCH subcarrier of data RE j of a symbol (nr_rxg_p of csrc/nr_rx_grid.h)"""
    return 2 * j + 1 if pattern == DMRS1 else (6 * (j // 4) + 2 + j % 4 if pattern == DMRS2 else j)


def rxg_count(pattern, N):
    """how many data REs of the pattern lie below subcarrier N"""
    n = 0
    while rxg_p(pattern, n) < N:
        n += 1
    return n


def extract(rx, ch, s):
    """[n, nb_re, 2] each: the REs and estimates of a grid segment (test_gpu_rx_grid.extract_np; an extracted segment's as they lie)"""
    if "pattern" not in s:
        return None if rx is None else rx[:, s["rx_off"]:s["rx_off"] + s["nb_re"]], ch[:, s["ch_off"]:s["ch_off"] + s["nb_re"]]
    idx = np.array([rxg_p(s["pattern"], j) for j in range(s["nb_re"])], np.int64)
    return None if rx is None else rx[:, s["rx_off"] + (s["start_re"] + idx) % s["fft_size"]], ch[:, s["ch_off"] + idx]


def draw_rx(rng, seams, kind):
    grid, two = kind != "front", kind in ("mmse", "ml")
    N = draw_fft(rng, seams) if grid else 0
    n_rx = int(rng.choice([2, 4])) if kind == "mmse" else int(rng.integers(1, 9))
    if grid:
        n_rx = min(n_rx, max(2 if kind == "mmse" else 1, RE_BUDGET // N))
        n_rx = 2 if kind == "mmse" and n_rx == 3 else n_rx
    seams.add(f"n_rx{n_rx}")
    n_ch = 2 * n_rx if two else n_rx
    n_tb = int(rng.integers(2, 4))
    seams.add(f"blocks{n_tb}")
    qms = [int(rng.choice(RX_QM[kind])) for _ in range(n_tb)]
    shift = np.array([pick(rng, SHIFT_SEAMS[kind], 0, 9 if two else 16)[0] for _ in range(n_tb)], np.int32)
    # the segments: block b takes at least one with REs (its measurement symbol)
    n_seg = int(rng.integers(n_tb, 9))
    tbs = list(range(n_tb)) + [int(rng.integers(0, n_tb)) for _ in range(n_seg - n_tb)]
    left, segs = RE_BUDGET // n_ch, []
    for i, tb in enumerate(tbs):
        pattern = int(rng.integers(0, 3)) if grid else FULL
        top = min(2600, left - max(0, n_tb - 1 - i), rxg_count(pattern, N) if grid else 1 << 30)
        nb = pick(rng, NB_SEAMS, 0, top)[0]
        if i < n_tb and nb == 0:
            nb = 1 + int(rng.integers(0, min(top, 40)))
        left -= nb
        s = dict(tb=tb, Qm=qms[tb], nb_re=nb)
        seams.add(f"Qm{qms[tb]}")
        seams.update(k for k, hit in (("nb0", nb == 0), ("nb1-7", 1 <= nb <= 7), ("nb1020-1028", 1020 <= nb <= 1028), ("nb2044-2052", 2044 <= nb <= 2052)) if hit)
        if grid:
            s.update(pattern=pattern, fft_size=N)
            seams.add(f"pattern{pattern}")
        segs.append(s)
    # the records: per block the segments' symbol ranges one after another in a drawn order, the blocks one after another
    rec_at = 2 * int(rng.integers(0, 4))
    for b in range(n_tb):
        mine = [s for s in segs if s["tb"] == b]
        offs, end = lay_out(rng, [s["nb_re"] for s in mine], int(rng.integers(0, 4)), 3)
        plane = (2 if two else 1) * end + int(rng.integers(0, 5))
        for s, o in zip(mine, offs):
            s.update(sym_off=o, plane=plane, rec_off=rec_at)
            seams.add(f"sym_res{o % 4}")
        rec_at += (qms[b] * plane if kind == "ml" else 2 * (qms[b] // 2) * plane) + 2 * int(rng.integers(0, 4))
    # the inputs
    if grid:
        n_slot = max(1, min(len(segs), RE_BUDGET // (N * n_rx)))
        ch_off, ch_end = lay_out(rng, [rxg_p(s["pattern"], s["nb_re"] - 1) + 1 if s["nb_re"] else 0 for s in segs], int(rng.integers(0, 8)), 3)
        for s, c in zip(segs, ch_off):
            s.update(rx_off=int(rng.integers(0, n_slot)) * (N + 1) + int(rng.integers(0, 3)), ch_off=c)
        rx_stride, ch_stride = n_slot * (N + 1) + 2 + int(rng.integers(0, 4)), ch_end + int(rng.integers(0, 4))
    else:
        rx_off, rx_end = lay_out(rng, [s["nb_re"] for s in segs], int(rng.integers(0, 4)), 3)
        ch_off, ch_end = lay_out(rng, [s["nb_re"] for s in segs], int(rng.integers(0, 4)), 3)
        for s, r, c in zip(segs, rx_off, ch_off):
            s.update(rx_off=r, ch_off=c)
        rx_stride = ch_stride = max(rx_end, ch_end) + int(rng.integers(0, 4))
    seams.add("odd_stride" if ch_stride & 1 else "even_stride")
    rx, ch = full_scale(rng, (n_rx, rx_stride, 2), 0.05), full_scale(rng, (n_ch, ch_stride, 2), 0.05)
    for b in range(n_tb):                                              # some blocks with a channel of moderate size
        if rng.random() < 0.5:
            seams.add("moderate_channel")
            for s in segs:
                if s["tb"] == b and s["nb_re"]:
                    ch[:, s["ch_off"]:s["ch_off"] + rxg_p(s.get("pattern", FULL), s["nb_re"] - 1) + 1] >>= 4 + b
    for s in segs:
        nb = s["nb_re"]
        seams.add(f"ch_res{s['ch_off'] % 4}")
        phase = 0 if two else (s["rec_off"] // 2 + s["sym_off"]) & 3     # the output arrays are 16-byte aligned, MARGIN a multiple of 4
        if not two:
            seams.add(f"phase{phase}")
            if -(-(nb + phase) // 1024) > -(-nb // 1024):                # rxf_place counts the groups from the aligned address
                seams.add("phase_adds_workgroup")
        groups = (nb + phase + 3) // 4
        seams.update(k for k, hit in (("two_workgroups", 256 < groups <= 512), ("three_workgroups", groups > 512)) if hit)
        if grid and nb:
            # the first RE behind the grid's wrap at every position of a thread's group, or no wrap at all
            how = rng.random()
            if how < 0.6 and nb > 1:
                w = int(rng.integers(1, nb))
                s["start_re"] = (N - rxg_p(s["pattern"], w)) % N
                seams.add(f"wrap_in_group{(w + phase) % 4}")
            else:
                s["start_re"] = 0 if how < 0.8 else int(rng.integers(0, max(1, N - rxg_p(s["pattern"], nb - 1))))
                seams.update(("no_wrap",) + (("start0",) if s["start_re"] == 0 else ()))
        elif grid:
            s["start_re"] = int(rng.integers(0, N))
    first = [next(s for s in segs if s["tb"] == b and s["nb_re"]) for b in range(n_tb)]
    first = [first[int(i)] for i in rng.permutation(n_tb)]
    segs = [segs[int(i)] for i in rng.permutation(len(segs))]
    d = dict(kind=kind, n_rx=n_rx, n_ch=n_ch, segs=segs, first=first, rx_stride=rx_stride, ch_stride=ch_stride,
             inputs=dict(rx=rx.reshape(-1), ch=ch.reshape(-1), shift=shift), outputs=dict(rec=(rec_at, np.int16, 1, CANARY), level=(n_tb, np.int32, 1, FILL32)))
    if kind == "mmse":
        nvar = np.array([0 if rng.random() < 0.4 else int(rng.integers(1, 80000)) for _ in range(n_tb)], np.uint32)
        d["inputs"]["nvar"] = nvar.view(np.int32)
        seams.update(("nvar0",) if (nvar == 0).any() else ())
        seams.update(("nvar_set",) if nvar.any() else ())
    if two:
        max_ch = np.array([pick(rng, (1500, 2047, 2048, 32767), 1, 32767)[0] for _ in range(n_tb)], np.int32)
        d["inputs"]["max_ch"] = max_ch
        seams.update(("max_ch_scaled",) if (max_ch >= 2048).any() else ())
        seams.update(("max_ch_plain",) if (max_ch < 2048).any() else ())
    d["small"] = sum(s["nb_re"] for s in segs) * n_ch <= 6000
    return d


def rx_arrays(d):
    i = d["inputs"]
    return i["rx"].reshape(d["n_rx"], d["rx_stride"], 2), i["ch"].reshape(d["n_ch"], d["ch_stride"], 2)


def rx_place(rec, d, s, out):
    """a segment's result into the records as the call's documentation lays them out"""
    import rx_ml_np
    import rx_mmse_np
    if d["kind"] == "mmse":
        rx_mmse_np.records_np(rec, out, s["Qm"], s["plane"], s["sym_off"], s["rec_off"])
    elif d["kind"] == "ml":
        rx_ml_np.llr_np(rec, out, s["Qm"], s["sym_off"], s["rec_off"])
    else:
        for k in range(s["Qm"] // 2):
            o = s["rec_off"] + 2 * (k * s["plane"] + s["sym_off"])
            rec[o:o + 2 * s["nb_re"]] = out[k].reshape(-1)


def rx_expected(m, d, model=False):
    """the host forms (model: the numpy restatements) segment by segment and block by block"""
    import rx_front_np
    import rx_ml_np
    import rx_mmse_np
    rx, ch = rx_arrays(d)
    kind, n_rx, inp = d["kind"], d["n_rx"], d["inputs"]
    rec = np.full(d["outputs"]["rec"][0], CANARY, np.int16)
    for s in d["segs"]:
        nb, sh = s["nb_re"], int(inp["shift"][s["tb"]])
        if nb == 0:
            continue
        if "pattern" in s and not model:                               # the library's own extraction, antenna by antenna
            parts = [m.ulsch_extract_host(rx[min(a, n_rx - 1), s["rx_off"]:], ch[a, s["ch_off"]:], s["pattern"], s["fft_size"], s["start_re"], nb)
                     for a in range(d["n_ch"])]
            a, b = np.stack([p[0] for p in parts[:n_rx]]), np.stack([p[1] for p in parts])
        else:
            a, b = extract(rx, ch, s)
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if kind == "mmse":
            nv = int(inp["nvar"].view(np.uint32)[s["tb"]])
            out = rx_mmse_np.mmse_np(a, b.reshape(2, n_rx, nb, 2), s["Qm"], sh, nv) if model else m.ulsch_mmse_2layers_host(a, b, n_rx, nb, nb, s["Qm"], sh, nv)
        elif kind == "ml":
            out = rx_ml_np.ml_np(a, b.reshape(2, n_rx, nb, 2), s["Qm"], sh) if model else m.ulsch_ml_2layers_host(a, b, n_rx, nb, nb, s["Qm"], sh)
        else:
            out = rx_front_np.compensate_np(a, b, s["Qm"], sh) if model else m.ulsch_compensate_host(a, b, n_rx, nb, nb, s["Qm"], sh)
        rx_place(rec, d, s, out)
    level = np.zeros(len(d["first"]), np.int32)
    for f in d["first"]:
        b, nb = np.ascontiguousarray(extract(None, ch, f)[1]), f["nb_re"]
        if kind == "mmse":
            mc = int(inp["max_ch"][f["tb"]])
            level[f["tb"]] = rx_mmse_np.level_mmse_np(b.reshape(2, n_rx, nb, 2), mc)[0] if model else m.ulsch_level_mmse_host(b, n_rx, nb, nb, mc)[0]
        elif kind == "ml":
            mc = int(inp["max_ch"][f["tb"]])
            level[f["tb"]] = rx_ml_np.level_ml_np(b.reshape(2, n_rx, nb, 2), mc)[0] if model else m.ulsch_level_ml_host(b, n_rx, nb, nb, mc)[0]
        else:
            level[f["tb"]] = rx_front_np.level_np(b)[0] if model else m.ulsch_level_host(b, n_rx, nb, nb)[0]
    return {"rec": embed(rec, 1), "level": embed(level, 1, FILL32)}


def rx_run(m, d, ins, outs):
    kind, n_rx = d["kind"], d["n_rx"]
    args = (ins["rx"], ins["ch"], n_rx, d["rx_stride"], d["ch_stride"], d["segs"], ins["shift"])
    if kind == "front":
        lv = m.ulsch_channel_level(ins["ch"], n_rx, d["ch_stride"], d["first"], out=outs["level"])
        m.ulsch_channel_compensation(ins["rx"], ins["ch"], n_rx, d["rx_stride"], d["segs"], ins["shift"], outs["rec"])
    elif kind == "grid":
        lv = m.ulsch_channel_level_grid(ins["ch"], n_rx, d["ch_stride"], d["first"], out=outs["level"])
        m.ulsch_channel_compensation_grid(*args, outs["rec"])
    elif kind == "mmse":
        lv = m.ulsch_channel_level_grid_mmse(ins["ch"], n_rx, d["ch_stride"], d["first"], ins["max_ch"], out=outs["level"])
        m.ulsch_mmse_2layers_grid(*args, ins["nvar"], outs["rec"])
    else:
        lv = m.ulsch_channel_level_grid_ml(ins["ch"], n_rx, d["ch_stride"], d["first"], ins["max_ch"], out=outs["level"])
        m.ulsch_ml_2layers_grid(*args, outs["rec"])
    if isinstance(ins["rx"], np.ndarray):                               # HOST mem returns the levels
        outs["level"][:len(d["first"])] = lv


# ---------------------------------------------------------------------------------------------------------
# PDSCH resource mapping, unit and precoded
# ---------------------------------------------------------------------------------------------------------
_pdm = ([f"pattern{k}" for k in range(3)] + ["ncdm1", "ncdm2", "l_prime0", "l_prime1"] + [f"Nl{k}" for k in range(1, 5)] + [f"n_tx{k}" for k in range(1, 9)]
        + ["amp32767"] + [f"tx_res{k}" for k in range(4)] + [f"sym_res{k}" for k in range(4)] + [f"rb{r}" for r in RB_SEAMS] + [f"fft{N}" for N in SIZES]
        + ["start_wrap", "two_pieces", "phase_adds_workgroup", "odd_stride", "even_stride", "zero_antennas"])
SEAMS["pdsch_map"] = _pdm
SEAMS["pdsch_precoded"] = _pdm + ["prg0", "prg2", "prg4", "prg_other", "pmi_zero_between", "prg_edge_in_group", "saturating"]


def draw_pdsch(rng, seams, precoded=False):
    """About one draw in sixteen is made from drawn allocations (d["allocs"]): each descriptor is then what pdsch_map_segments makes
    of a one- or two-symbol allocation -- c_init from slot, symbol, scrambling identity and scid, dmrs_offset from the first PRB,
    the ports in ascending order -- laid out as every other draw is, and small enough for pdsch_map_np.py / pdsch_precode_np.py,
    which work on allocations (pdsch_modelled)."""
    import pdsch_map_np
    import test_gpu_pdsch_map as GPM
    from_alloc = rng.random() < 1 / 16
    N0 = draw_fft(rng, seams)
    if from_alloc and N0 > 1536:
        seams.discard(f"fft{N0}")
        N0 = int(rng.choice(SIZES[:5]))
    Nl = int(rng.integers(1, 5))
    n_tx = max(Nl, min(int(rng.integers(1, 9)), max(1, RE_BUDGET // N0)))
    seams.update((f"Nl{Nl}", f"n_tx{n_tx}") + (("zero_antennas",) if n_tx > Nl else ()))
    n_seg = int(rng.integers(1, 1 + max(1, min(3 if from_alloc else 8, RE_BUDGET // (N0 * n_tx)))))
    slot, segs, lay_at, allocs = N0 + 4, [], int(rng.integers(0, 4)), []
    for i in range(n_seg):
        N = N0 if i == 0 or rng.random() < 0.6 else int(rng.choice([s for s in SIZES if s <= N0]))
        seams.add(f"fft{N}")
        pattern, ncdm = [(FULL, 0), (DMRS1, 1), (DMRS1, 2), (DMRS2, 1), (DMRS2, 2), (DMRS2, 3)][int(rng.integers(0, 6))]
        ports, per_rb = GPM.PORTS[(pattern, ncdm)]
        # 256 PRBs are 3 * 1024 REs: the one width at which the write phase adds a workgroup, so it is drawn more often
        rb = pick(rng, RB_SEAMS + ((256,) * 6 + (257,) * 3 if N >= 4096 else ()), 1, N // 12)[0]
        rb = min(rb, 12) if from_alloc else rb
        k0 = pick(rng, [0, N - 1, N - 2] + [(N - 6 * rb + j) % N for j in range(-2, 3)], 0, N - 1)[0]
        nb_re, sym_off = per_rb * rb, int(rng.integers(0, 8))
        plane = sym_off + nb_re + int(rng.integers(0, 3))
        l_prime = int(rng.integers(0, 2)) if pattern else 0
        amp = pick(rng, (1, 512, 32767, 9000), 1, 32767)[0]
        tx_off = i * slot + int(rng.integers(0, 4))
        port = [ports[int(k)] for k in rng.permutation(4)[:Nl]] if pattern else []
        dmrs_offset, c_init = (int(rng.integers(0, 1901)), int(rng.integers(0, 1 << 31))) if pattern else (0, 0)
        if from_alloc:
            # the symbol of an l' = 1 descriptor is the second of a DMRS pair; the reference wraps start_sc once: first PRB below N / 12
            al = dict(slot=int(rng.integers(0, 20)), symbol=int(rng.integers(1, 13)), nid=int(rng.integers(0, 1 << 16)), scid=int(rng.integers(0, 2)),
                      rb_start=int(rng.integers(0, 4)), bwp_start=int(rng.integers(0, N // 12 - 3)))
            allocs.append(al)
            port = sorted(port)
            if pattern:
                dmrs_offset = (al["rb_start"] + al["bwp_start"]) * (6 if pattern == DMRS1 else 4)
                c_init = pdsch_map_np.c_init_pdsch(al["slot"], al["symbol"], al["nid"], al["scid"])
        segs.append(dict(pattern=pattern, Nl=Nl, ncdm=ncdm, l_prime=l_prime, port=port, amp=amp, fft_size=N, start_re=k0, rb_size=rb, nb_re=nb_re, sym_off=sym_off,
                         plane=plane, dmrs_offset=dmrs_offset, c_init=c_init, tx_off=tx_off, lay_off=2 * lay_at))
        lay_at += Nl * plane + int(rng.integers(0, 3))
        seams.update((f"pattern{pattern}", f"sym_res{sym_off % 4}", f"tx_res{(tx_off + k0) % 4}"))
        seams.update(k for k, hit in ((f"ncdm{ncdm}", pattern and ncdm < 3), (f"l_prime{l_prime}", pattern), ("amp32767", amp == 32767), (f"rb{rb}", rb in RB_SEAMS),
                                      ("start_wrap", k0 + 12 * rb > N), ("two_pieces", 12 * rb > 1024)) if hit)
    stride = n_seg * slot + int(rng.integers(0, 5))
    seams.add("odd_stride" if stride & 1 else "even_stride")
    for s in segs:                                                     # the grid array is 16-byte aligned, MARGIN a multiple of 4
        for a in range(n_tx):
            phase, n_re = (s["tx_off"] + a * stride + s["start_re"]) & 3, 12 * s["rb_size"]
            if -(-(n_re + phase) // 1024) > -(-n_re // 1024):
                seams.add("phase_adds_workgroup")
    lay = full_scale(rng, (lay_at + 4, 2), 0.15)
    d = dict(n_tx=n_tx, segs=segs, stride=stride, inputs=dict(lay=lay), outputs=dict(tx=(n_tx * stride, np.int16, 2, CANARY)), small=from_alloc)
    if from_alloc:
        d["allocs"] = allocs
    if precoded:
        import test_gpu_pdsch_precode as GPP
        table = GPP.table_for(rng, Nl)
        if from_alloc:                                                 # the restatement finds matrix pmi at entry pmi - 1
            table = [dict(t, pm_idx=k + 1) for k, t in enumerate(table)]
        idx = [t["pm_idx"] for t in table]
        prgs, pmis = [], [idx[0]]
        for s in segs:
            size = pick(rng, (0, 2, 4, s["rb_size"]), 0, s["rb_size"])[0]
            n = -(-s["rb_size"] // size) if size else 0
            mine = [0 if n_tx < 2 or rng.random() < 0.35 else int(rng.choice(idx)) for _ in range(n)]
            prgs.append(dict(prg_size=size, pmi_off=len(pmis), pmi_count=n))
            pmis += mine
            seams.add({0: "prg0", 2: "prg2", 4: "prg4"}.get(size, "prg_other"))
            if any(mine[q] == 0 and mine[q - 1] and mine[q + 1] for q in range(1, n - 1)):
                seams.add("pmi_zero_between")
            if idx[2] in mine and Nl > 1:
                seams.add("saturating")
        if GPP.prg_edges_inside_groups(segs, prgs, pmis, stride, n_tx):
            seams.add("prg_edge_in_group")
        d.update(prgs=prgs, pmis=pmis, table=table)
    return d


def pdsch_order(rng, d):
    order = [int(i) for i in rng.permutation(len(d["segs"]))]
    d["segs"] = [d["segs"][i] for i in order]
    for k in ("prgs", "allocs"):
        if k in d:
            d[k] = [d[k][i] for i in order]
    return d


def pdsch_modelled(m, d):
    """pdsch_map_np.py (and pdsch_precode_np.py behind it) on the allocation of every descriptor, the symbol of the descriptor taken
    out of the restatement's slot and put where the descriptor writes; the allocation's own descriptor, as the library derives it,
    must be the drawn one"""
    import pdsch_precode_np as pre
    from test_pdsch_map_host import FILL, alloc, run_ref
    lay, n_tx, stride = d["inputs"]["lay"], d["n_tx"], d["stride"]
    tx = np.full((n_tx * stride, 2), CANARY, np.int16)
    for i, (s, al) in enumerate(zip(d["segs"], d["allocs"])):
        N, Nl, nb, lp = s["fft_size"], s["Nl"], s["nb_re"], s["l_prime"]
        sym, first = al["symbol"], al["symbol"] - lp
        ports = sum(1 << p for p in s["port"]) if s["pattern"] else (1 << Nl) - 1
        a = alloc(max(s["pattern"] - 1, 0), ports, max(s["ncdm"], 1), N, s["rb_size"], s["start_re"], s["amp"], ((3 if lp else 1) << first) if s["pattern"] else 0,
                  first, 1 + lp, Nl=Nl, rb_start=al["rb_start"], bwp_start=al["bwp_start"], slot=al["slot"], nid=al["nid"], scid=al["scid"], plane=(1 + lp) * nb)
        mine = m.pdsch_map_segments([a])[-1]
        keys = ("pattern", "Nl", "l_prime", "amp", "fft_size", "start_re", "rb_size", "nb_re") + (("ncdm", "dmrs_offset", "c_init") if s["pattern"] else ())
        assert all(mine[k] == s[k] for k in keys) and (not s["pattern"] or mine["port"][:Nl] == s["port"]), (d["seed"], i, mine, s)
        planes = np.zeros((Nl, a["plane"], 2), np.int16)                 # the symbol in front of an l' = 1 symbol consumes nb entries
        for l in range(Nl):
            at = s["lay_off"] // 2 + l * s["plane"] + s["sym_off"]
            planes[l, a["plane"] - nb:] = lay[at:at + nb]
        if "prgs" in d:
            g = d["prgs"][i]
            mapped = [[[tuple(int(v) for v in c) for c in sy] for sy in layer] for layer in run_ref(a, planes, Nl, literal_tail=False, literal_allowed=False)[0]]
            table = [dict(t, weights=[[tuple(int(v) for v in w) for w in row] for row in np.asarray(t["weights"])]) for t in d["table"]]
            want = np.array(pre.precode_all_simd(a, mapped, n_tx, g["prg_size"], d["pmis"][g["pmi_off"]:g["pmi_off"] + g["pmi_count"]], table, fill=FILL)[0],
                            np.int64).astype(np.int16)
        else:
            want = run_ref(a, planes, n_tx, literal_tail=False, literal_allowed=False)[0]
        idx = (s["start_re"] + np.arange(12 * s["rb_size"])) % N
        rest = np.ones(N, bool)
        rest[idx] = False
        assert (want[:, sym, rest] == CANARY).all(), "the restatement writes the allocation's REs and nothing else"
        for ant in range(n_tx):
            tx[s["tx_off"] + ant * stride + idx] = want[ant, sym, idx]
    return {"tx": embed(tx, 2)}


def pdsch_expected(m, d):
    import test_gpu_pdsch_map as GPM
    import test_gpu_pdsch_precode as GPP
    lay = d["inputs"]["lay"]
    if "prgs" in d:
        return {"tx": embed(GPP.host_form(m, d["segs"], d["prgs"], d["pmis"], d["table"], lay, d["stride"], d["n_tx"]), 2)}
    return {"tx": embed(GPM.host_form(m, d["segs"], lay, d["stride"], d["n_tx"]), 2)}


def pdsch_run(m, d, ins, outs):
    if "prgs" in d:
        m.pdsch_resource_mapping_precoded(ins["lay"], outs["tx"], d["stride"], d["n_tx"], d["segs"], d["prgs"], d["pmis"], d["table"])
    else:
        m.pdsch_resource_mapping(ins["lay"], outs["tx"], d["stride"], d["n_tx"], d["segs"])


# ---------------------------------------------------------------------------------------------------------
KINDS = {
    "front": (lambda rng, seams: draw_rx(rng, seams, "front"), rx_expected, rx_run, lambda m, d: rx_expected(m, d, model=True)),
    "grid": (lambda rng, seams: draw_rx(rng, seams, "grid"), rx_expected, rx_run, lambda m, d: rx_expected(m, d, model=True)),
    "mmse": (lambda rng, seams: draw_rx(rng, seams, "mmse"), rx_expected, rx_run, lambda m, d: rx_expected(m, d, model=True)),
    "ml": (lambda rng, seams: draw_rx(rng, seams, "ml"), rx_expected, rx_run, lambda m, d: rx_expected(m, d, model=True)),
    "pdsch_map": (lambda rng, seams: pdsch_order(rng, draw_pdsch(rng, seams)), pdsch_expected, pdsch_run, pdsch_modelled),
    "pdsch_precoded": (lambda rng, seams: pdsch_order(rng, draw_pdsch(rng, seams, precoded=True)), pdsch_expected, pdsch_run, pdsch_modelled),
    "chest": (lambda rng, seams: chest_order(rng, draw_chest(rng, seams)), chest_expected, chest_run, chest_modelled),
    "chest_meas": (lambda rng, seams: chest_order(rng, draw_chest(rng, seams, meas=True)), chest_expected, chest_run, chest_modelled),
    "time_avg": (draw_time_avg, time_avg_expected, time_avg_run, time_avg_modelled),
    "delay": (draw_delay, delay_expected, delay_run, delay_modelled),
}


def draw(call, seed):
    rng = np.random.default_rng([CALLS.index(call), seed])
    seams = set()
    d = KINDS[call][0](rng, seams)
    for a in d["inputs"].values():
        if a is not None:
            a.setflags(write=False)
    assert seams <= set(SEAMS[call]), seams - set(SEAMS[call])
    return dict(d, call=call, seed=seed, seams=seams)


def expected(m, d):
    return KINDS[d["call"]][1](m, d)


def run(m, d, ins, outs):
    return KINDS[d["call"]][2](m, d, ins, outs)


def modelled(m, d):
    return KINDS[d["call"]][3](m, d)


def fresh_outputs(d):
    """the output arrays of a draw with their margins, canary-filled (an in-place call's array holds its input between them)"""
    outs = {}
    for name, (n, dtype, width, fill) in d["outputs"].items():
        outs[name] = with_margin(n, dtype, width, fill)
        if name in d.get("init", {}):
            inner(outs[name], width)[:n * width] = d["init"][name].reshape(-1)
    return outs


def tally(call, seeds):
    """how often each seam category of `call` is hit over `seeds`"""
    t = {s: 0 for s in SEAMS[call]}
    for seed in seeds:
        for s in draw(call, seed)["seams"]:
            t[s] += 1
    return t
