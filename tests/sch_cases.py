"""The transport blocks test_sch_model_host.py and test_gpu_sch_model.py share.  Every one is found by searching with sch_np's own
quantities for an edge of TS 38.212 (edges_of() below names them); none is typed in from the oracle or from csrc/.  Apart from the
sizes the thresholds of 5.2.2 and 7.2.1 force (A = 3824 / 3832, B around Kcb, three blocks), everything stays at Zc <= 64."""
import numpy as np

import sch_np as S

QMNL = [(8, 4), (6, 4), (8, 3), (6, 3), (4, 4), (8, 2), (4, 3), (6, 2), (2, 4), (4, 2), (8, 1), (2, 3), (6, 1), (4, 1), (2, 2), (2, 1)]


def lbrm_for(ncb, C):
    """a TBS_LBRM with floor(3 T / (2 C)) = ncb, or None where there is none"""
    T = -(-2 * C * ncb // 3)
    return T if (3 * T) // (2 * C) == ncb else None


def selection(tb):
    """per block, the indices into d in the order of selection (e_0 .. e_(E-1))"""
    p = S.plan(tb)
    null = np.zeros(p["N"], bool)
    null[p["fs"]:p["fe"]] = True
    return p, [S.select(null, p["Ncb"], p["k0"], E, p["N"]) for E in p["E"]]


def edges_of(tb):
    """the names of the edges a transport block sits on, from the model's quantities alone"""
    p, sel = selection(tb)
    BG, B, Zc, Ncb, k0, fs, fe, V = tb["BG"], p["B"], p["Zc"], p["Ncb"], p["k0"], p["fs"], p["fe"], p["V"]
    lb = "LBRM" if Ncb < p["N"] else "full"
    out = {"iLS %d BG%d" % (p["iLS"], BG), "rv %d %s" % (tb["rv"], lb), "Qm %d" % tb["Qm"], "Nl %d" % tb["Nl"]}
    def add(cond, name):
        if cond:
            out.add(name)
    add(tb["A"] == 3824 and p["Ltb"] == 16, "CRC16 at A = 3824")
    add(tb["A"] == 3832 and p["Ltb"] == 24, "CRC24A at A = 3832")
    add(p["C"] == 1 and S.KCB[BG] - 8 < B <= S.KCB[BG], "C = 1 at Kcb BG%d" % BG)
    add(p["C"] == 2 and S.KCB[BG] < B <= S.KCB[BG] + 16, "C = 2 just above Kcb BG%d" % BG)
    add(p["C"] >= 3 and len(set(p["E"])) == 2, "C >= 3 with two E sizes")
    for t in (192, 560, 640):
        add(BG == 2 and B == t, "BG2 B = %d" % t)
        add(BG == 2 and t < B <= t + 8, "BG2 B just above %d" % t)
    add(p["Kb"] * Zc == p["Kp"], "Kb Zc = K'")
    add(p["Kb"] * Zc - p["Kp"] == 8, "Kb Zc = K' + 8")
    add(p["F"] % 8 != 0, "F no multiple of 8")
    add(p["F"] > 0 and fs < k0 < fe, "k0 inside the fillers BG%d" % BG)
    add(p["F"] > 0 and k0 == fs, "k0 at the filler start BG%d" % BG)
    add(p["F"] > 0 and k0 == fe, "k0 at the filler end BG%d" % BG)
    add(Ncb % 2 == 1, "Ncb odd")
    add(Ncb % 8 == 4, "Ncb = 4 mod 8")
    add(Ncb % 8 == 0 and Ncb % Zc != 0, "Ncb multiple of 8, not of Zc")
    add(Zc == 384, "Zc = 384")
    for E, s in zip(p["E"], sel):
        last = int(s[-1])
        add(E < Ncb - k0 and k0 > 0, "E < Ncb - k0")
        add(last == Ncb - 1 and k0 > 0, "ends exactly at Ncb")
        add(p["F"] > 0 and last == fs - 2 and E > V, "wraps and ends one before the filler start")
        add(p["F"] > 0 and last == fs - 1 and E > V, "wraps and ends at the filler start")
        add(p["F"] > 0 and last == fe and E > V, "wraps and ends one past the fillers")
        add(E > 3 * V, "E above 3 laps")
    return out


ALL_EDGES = (
    ["iLS %d BG%d" % (i, bg) for i in range(8) for bg in (1, 2)] + ["rv %d %s" % (rv, lb) for rv in range(4) for lb in ("LBRM", "full")] +
    ["Qm %d" % q for q in (2, 4, 6, 8)] + ["Nl %d" % n for n in (1, 2, 3, 4)] +
    ["CRC16 at A = 3824", "CRC24A at A = 3832", "C >= 3 with two E sizes", "Kb Zc = K'", "Kb Zc = K' + 8", "Ncb odd", "Ncb = 4 mod 8",
     "Ncb multiple of 8, not of Zc", "Zc = 384", "E < Ncb - k0", "ends exactly at Ncb", "wraps and ends one before the filler start",
     "wraps and ends at the filler start", "wraps and ends one past the fillers", "E above 3 laps"] +
    ["%s BG%d" % (n, bg) for n in ("C = 1 at Kcb", "C = 2 just above Kcb", "k0 inside the fillers", "k0 at the filler start", "k0 at the filler end")
     for bg in (1, 2)] + ["BG2 B = %d" % t for t in (192, 560, 640)] + ["BG2 B just above %d" % t for t in (192, 560, 640)])


def sizes_of(A, BG):
    return S.segment_sizes(A + S.tb_crc_len(A), BG)


def contract_sizes(BG, lo, hi):
    """(A, sizes) for every A in [lo, hi) that meets the library's byte contract"""
    for A in range(lo, hi, 8):
        try:
            s = sizes_of(A, BG)
        except ValueError:
            continue
        if s["byte_contract"]:
            yield A, s


def tb_of(A, BG, E, Qm=2, Nl=1, rv=0, ncb=None):
    """a transport block whose every code block gets E bits"""
    s = sizes_of(A, BG)
    T = 0
    if ncb is not None:
        T = lbrm_for(ncb, s["C"])
        assert T is not None
    assert E % (Qm * Nl) == 0
    return dict(A=A, G=s["C"] * E, BG=BG, Qm=Qm, Nl=Nl, rv=rv, tbslbrm=T)


def fit(E):
    """the largest Qm Nl that divides E, or None"""
    for Qm, Nl in QMNL:
        if E % (Qm * Nl) == 0:
            return Qm, Nl
    return None


def count_to(p, last, laps=0):
    """E whose last selected index is `last`, after `laps` whole laps more"""
    t = np.ones(p["Ncb"], bool)
    t[p["fs"]:p["fe"]] = False
    assert t[last]
    k0 = p["k0"]
    first = int(t[k0:last + 1].sum()) if last >= k0 else int(t[k0:].sum() + t[:last + 1].sum())
    return first + laps * p["V"]


def build():
    cases = []

    def put(name, tb):
        if not any(tb == c["tb"] for c in cases):
            cases.append(dict(name=name, tb=tb))

    rate = lambda s, q=1: -(-int(2.2 * s["Kp"]) // q) * q
    # -- the thresholds of 7.2.1 and 5.2.2
    for BG in (1, 2):
        for A in (3824, 3832):
            put("A = %d BG%d" % (A, BG), tb_of(A, BG, rate(sizes_of(A, BG), 2)))
        allA = list(contract_sizes(BG, 3000, 8600 if BG == 1 else 7800))
        A1 = max(A for A, s in allA if s["C"] == 1)
        A2 = min(A for A, s in allA if s["C"] == 2)
        put("largest C = 1 BG%d" % BG, tb_of(A1, BG, rate(sizes_of(A1, BG), 4), Qm=4))
        put("smallest C = 2 BG%d" % BG, tb_of(A2, BG, rate(sizes_of(A2, BG), 4), Qm=4))
    A3, s3 = min((A, s) for A, s in contract_sizes(2, 7000, 7800) if s["C"] == 3)
    q = 3 * (rate(s3, 12) // 12) + 1                                   # G / (Nl Qm) = 1 mod 3: blocks 0 and 1 short, block 2 long
    put("three blocks, two E", dict(A=A3, G=12 * q, BG=2, Qm=6, Nl=2, rv=0, tbslbrm=0))
    A2, s2 = min((A, s) for A, s in contract_sizes(2, 3800, 4200) if s["C"] == 2)   # two blocks under LBRM, TBS_LBRM odd: C enters N_ref
    ncb = next(n for n in range(s2["K"] + 9 * s2["Zc"] + 1, s2["N"]) if (lbrm_for(n, 2) or 0) % 2 == 1 and (3 * (lbrm_for(n, 2) // 2)) // 2 != n)
    put("two blocks under LBRM", tb_of(A2, 2, rate(s2, 8), Qm=4, Nl=2, rv=1, ncb=ncb))
    small2 = list(contract_sizes(2, 24, 800))
    for t in (192, 560, 640):
        below = max(A for A, s in small2 if s["B"] <= t)
        above = min(A for A, s in small2 if s["B"] > t)
        for A in (below, above):
            put("BG2 B = %d" % sizes_of(A, 2)["B"], tb_of(A, 2, rate(sizes_of(A, 2), 2)))
    for BG in (1, 2):
        small = list(contract_sizes(BG, 24, 1500 if BG == 1 else 640))
        A0 = min(A for A, s in small if s["Kb"] * s["Zc"] == s["Kp"] and s["Zc"] >= 8)
        A8 = min(A for A, s in small if s["Kb"] * s["Zc"] - s["Kp"] == 8 and s["Zc"] >= 8)
        put("Kb Zc = K' BG%d" % BG, tb_of(A0, BG, rate(sizes_of(A0, BG), 8), Qm=8))
        put("Kb Zc = K' + 8 BG%d" % BG, tb_of(A8, BG, rate(sizes_of(A8, BG), 8), Qm=8))
        for i in range(8):                                             # every set index, at the second-smallest size that has it
            As = [A for A, s in small if s["iLS"] == i and s["Zc"] <= 64]
            A = As[min(1, len(As) - 1)]
            Qm, Nl = QMNL[(3 * i + BG) % len(QMNL)]
            put("iLS %d BG%d" % (i, BG), tb_of(A, BG, rate(sizes_of(A, BG), Qm * Nl), Qm=Qm, Nl=Nl, rv=i % 4))
    # -- rv 0 - 3 with and without LBRM, every Qm and Nl
    n = 0
    for BG, lo in ((1, 400), (2, 296)):
        A, s = next(iter(contract_sizes(BG, lo, lo + 400)))
        for rv in range(4):
            for ncb in (None, (s["K"] - 2 * s["Zc"]) + 11 * s["Zc"] + 5):
                Qm, Nl = (2, 4, 6, 8)[n % 4], 1 + (n // 4 + n) % 4
                if ncb is not None:
                    while lbrm_for(ncb, s["C"]) is None:
                        ncb += 1
                put("rv %d BG%d" % (rv, BG), tb_of(A, BG, rate(s, Qm * Nl), Qm=Qm, Nl=Nl, rv=rv, ncb=ncb))
                n += 1
    # -- k0 inside the filler range, at its start and at its end; the search runs over A, rv and Ncb
    for BG in (1, 2):
        want = {"k0 inside the fillers BG%d" % BG, "k0 at the filler start BG%d" % BG, "k0 at the filler end BG%d" % BG}
        for A, s in contract_sizes(BG, 24, 400):
            if not want:
                break
            if s["F"] == 0 or s["Zc"] > 64:
                continue
            fs, fe = s["Kp"] - 2 * s["Zc"], s["K"] - 2 * s["Zc"]
            for rv in (1, 2, 3):
                for ncb in range(fe, s["N"] + 1):
                    k0 = S.k0_of(BG, s["Zc"], ncb, rv)
                    hit = ("k0 inside the fillers BG%d" % BG if fs < k0 < fe else "k0 at the filler start BG%d" % BG if k0 == fs else
                           "k0 at the filler end BG%d" % BG if k0 == fe else None)
                    if hit in want and lbrm_for(ncb, s["C"]) is not None:
                        want.discard(hit)
                        put(hit, tb_of(A, BG, rate(s, 2), rv=rv, ncb=ncb))
        assert not want, want
    # -- the circular buffer's length: odd, 4 mod 8, a multiple of 8 but not of Zc
    A, s = next((A, s) for A, s in contract_sizes(1, 200, 600) if s["Zc"] % 2 == 1 and s["F"] % 8)
    fe = s["K"] - 2 * s["Zc"]
    for name, ok, rv in (("Ncb odd", lambda n: n % 2 == 1, 1), ("Ncb = 4 mod 8", lambda n: n % 8 == 4, 2),
                         ("Ncb multiple of 8, not of Zc", lambda n: n % 8 == 0 and n % s["Zc"], 3)):
        ncb = next(n for n in range(fe + 3 * s["Zc"], s["N"]) if ok(n) and lbrm_for(n, 1) is not None)
        put(name, tb_of(A, 1, rate(s, 4), Qm=4, rv=rv, ncb=ncb))
    # -- where the selection ends
    for BG, rv, lbrm in ((1, 1, False), (2, 2, True), (1, 3, True), (2, 1, False)):
        done = set()
        for A, s in contract_sizes(BG, 120, 900):
            if s["F"] < 8 or s["Zc"] > 64:
                continue
            ncb = None
            if lbrm:
                ncb = s["N"] - 7 * s["Zc"] - 3
                while lbrm_for(ncb, 1) is None:
                    ncb += 1
            p = S.plan(tb_of(A, BG, 2 * s["Kp"], rv=rv, ncb=ncb))
            targets = {"short": (p["Ncb"] - p["k0"]) // 2 // 2 * 2, "at Ncb": count_to(p, p["Ncb"] - 1), "at Ncb + 1 lap": count_to(p, p["Ncb"] - 1, 1),
                       "fs - 1": count_to(p, p["fs"] - 2, 0 if p["k0"] > p["fs"] else 1), "fs": count_to(p, p["fs"] - 1, 0 if p["k0"] > p["fs"] else 1),
                       "fe + 1": count_to(p, p["fe"], 0 if p["k0"] > p["fe"] else 1), "laps": 3 * p["V"] + 2 * ((p["Zc"] + 1) // 2) + 2}
            for key, E in targets.items():
                if key in done or E < p["fs"] or fit(E) is None:
                    continue
                Qm, Nl = fit(E)
                done.add(key)
                put("%s BG%d rv%d" % (key, BG, rv), tb_of(A, BG, E, Qm=Qm, Nl=Nl, rv=rv, ncb=ncb))
            if len(done) == 7:
                break
        assert len(done) >= 5, (BG, rv, done)                         # (late rv: what is left before Ncb is shorter than the library takes)
    return cases


CASES = build()
for _i, _c in enumerate(CASES):
    _c["id"] = "%02d %s" % (_i, _c["name"])



def refused():
    """what the library refuses by its documented contract (nr_hip_rate_match_geometry) although 5.4.2.1 defines it, one block per
    kind: E below the first filler; a circular buffer that ends before the fillers; one that ends inside them.  Held on the
    refusal of the call and of the CPU emulation, and on the model giving G bits."""
    tb = CASES[-1]["tb"]
    p = S.plan(dict(tb, tbslbrm=0))
    assert p["C"] == 1 and 8 < p["fs"] < p["fe"] < p["N"]
    E = 2 * (p["fe"] // 2) + 8                                         # (not the first kind: E > fs)
    before = next(n for n in range(p["fs"] - 1, 0, -1) if lbrm_for(n, 1) is not None)
    inside = next(n for n in range((p["fs"] + p["fe"]) // 2, p["fe"]) if lbrm_for(n, 1) is not None)
    base = dict(A=tb["A"], BG=tb["BG"], Qm=2, Nl=1, rv=0)
    return [dict(base, kind="E below the first filler", G=8, tbslbrm=0),
            dict(base, kind="Ncb before the fillers", G=E, tbslbrm=lbrm_for(before, 1)),
            dict(base, kind="Ncb inside the fillers", G=E, tbslbrm=lbrm_for(inside, 1))]


REFUSED = refused()
