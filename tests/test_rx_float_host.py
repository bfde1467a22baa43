"""The three UL receivers' soft outputs against float64 detectors (rx_float_np.py), on the CPU: the numpy restatements of the
reference (rx_front_np.py + qam_np.py, rx_mmse_np.py, rx_ml_np.py) and the library's CPU forms (ulsch_compensate_host + demap_np,
ulsch_mmse_2layers_host, ulsch_ml_2layers_host) on channels whose layers are coupled (correlation 0, 0.5, 0.8, 0.95), at two noise
levels, every RE of every case.  The bit-exact tests compare the library with restatements written from the same reference lines;
this one compares both with numbers computed another way.

The bounds (rx_float_np.BOUNDS) are the restatement's worst deviation from the model over the case list, times 1.5, rounded up;
the test checks that the table says what it measures.  For each deliberate misreading of rx_float_np.MUTATIONS the restatement
must miss the misread model by more than twice the bound on some case, and the set of cases that notice it is pinned (NOTICED).
With c = 0 alone the misreadings of the coupling terms go unnoticed: that is why the cases with c > 0 exist."""
import functools
import math

import numpy as np
import pytest

import rx_float_np as F
import rx_ml_np as RML
from qam_np import demap_np
from rx_front_np import compensate_np, level_np
from rx_ml_np import level_ml_np, ml_np
from rx_mmse_np import level_mmse_np, mmse_np

RECEIVERS = ("single", "mmse", "ml")
MEAS = slice(sum(F.SEGMENTS) - F.SEGMENTS[-1], sum(F.SEGMENTS))        # the measurement symbol: the last segment
COUPLING = {"mmse": ("b_c_exchanged",), "ml": ("rho_conjugated", "rho_exchanged", "a_sq_dropped", "interference_abs_inverted")}


@functools.lru_cache(maxsize=None)
def cases(receiver):
    return F.case_list(receiver)


def variants(receiver, cs):
    """the runs of a case: (key, extra arguments)"""
    if receiver == "mmse":
        return [(f"{cs['name']}-nvar{'0' if nv == 0 else '+'}", (nv,)) for nv in F.nvars_of(cs)]
    return [(cs["name"], ())]


def level_of(receiver, cs, m=None):
    """the shift out of the receiver's own level formula on the measurement symbol"""
    n_rx, nb = cs["n_rx"], F.SEGMENTS[-1]
    if receiver == "single":
        ch = np.ascontiguousarray(cs["ch"][0][:, MEAS])
        return int(m.ulsch_level_host(ch, n_rx, nb, nb)[0]) if m else int(level_np(ch)[0])
    ch = np.ascontiguousarray(cs["ch"][:, :, MEAS])
    if receiver == "mmse":
        return int(m.ulsch_level_mmse_host(ch, n_rx, nb, nb, cs["max_ch"])[0]) if m else int(level_mmse_np(ch, cs["max_ch"])[0])
    return int(m.ulsch_level_ml_host(ch, n_rx, nb, nb, cs["max_ch"])[0]) if m else int(level_ml_np(ch, cs["max_ch"])[0])


def demapped(planes, Qm):
    """int16 [nb_re, Qm] of a layer's y and magnitude planes"""
    return demap_np(planes[0], list(planes[1:]), Qm).reshape(-1, Qm).astype(np.int64)


def receiver_llrs(receiver, cs, lv, extra=(), m=None, planes_out=None):
    """int64 [n, Qm] (single) or [n, 2, Qm]: the restatement's (m = None) or the CPU form's LLRs, segment by segment"""
    Qm, n_rx, out = cs["Qm"], cs["n_rx"], []
    for at, nb in F.segments_of(cs):
        if receiver == "single":
            rx, ch = np.ascontiguousarray(cs["rx1"][:, at:at + nb]), np.ascontiguousarray(cs["ch"][0][:, at:at + nb])
            pl = m.ulsch_compensate_host(rx, ch, n_rx, nb, nb, Qm, lv) if m else compensate_np(rx, ch, Qm, lv)
            out.append(demapped(pl, Qm))
        else:
            rx, ch = np.ascontiguousarray(cs["rx"][:, at:at + nb]), np.ascontiguousarray(cs["ch"][:, :, at:at + nb])
            if receiver == "mmse":
                pl = m.ulsch_mmse_2layers_host(rx, ch, n_rx, nb, nb, Qm, lv, extra[0]) if m else mmse_np(rx, ch, Qm, lv, extra[0])
                out.append(np.stack([demapped(pl[l], Qm) for l in range(2)], 1))
            else:
                pl = None
                out.append((m.ulsch_ml_2layers_host(rx, ch, n_rx, nb, nb, Qm, lv) if m else ml_np(rx, ch, Qm, lv)).astype(np.int64))
        if planes_out is not None:
            planes_out.append(pl)
    return np.concatenate(out)


def model_llrs(receiver, cs, lv, extra=(), **kw):
    """float64, the shape of receiver_llrs"""
    out = []
    for at, nb in F.segments_of(cs):
        if receiver == "single":
            out.append(F.single_layer(cs["rx1"][:, at:at + nb], cs["ch"][0][:, at:at + nb], cs["Qm"], lv, **kw))
        elif receiver == "mmse":
            out.append(F.mmse(cs["rx"][:, at:at + nb], cs["ch"][:, :, at:at + nb], cs["Qm"], lv, extra[0], **kw)[0])
        else:
            out.append(F.ml(cs["rx"][:, at:at + nb], cs["ch"][:, :, at:at + nb], cs["Qm"], lv, **kw))
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def restated(receiver):
    """key -> (case, extra, lv, the restatement's LLRs), computed once and left unchanged"""
    out = {}
    for cs in cases(receiver):
        lv = level_of(receiver, cs)
        for key, extra in variants(receiver, cs):
            got = receiver_llrs(receiver, cs, lv, extra)
            got.setflags(write=False)
            out[key] = (cs, extra, lv, got)
    return out


def deviations(receiver, **kw):
    """key -> the largest |restatement - model| over every RE, layer and bit of the run"""
    return {key: float(np.abs(got - model_llrs(receiver, cs, lv, extra, **kw)).max()) for key, (cs, extra, lv, got) in restated(receiver).items()}


def bound_of(receiver, cs):
    return F.BOUNDS[(receiver, cs["Qm"])][1]


# ---- the model by itself ---------------------------------------------------------------------------------------------------
def test_model_constellations_and_its_two_forms_agree():
    for Qm in (2, 4, 6, 8):
        x = F.points(Qm)
        assert abs((np.abs(x) ** 2).mean() - 1.0) < 1e-12 and len(set(np.round(x, 9))) == 1 << Qm
        lev = np.unique(np.round(x.real * np.sqrt(F.NORM[Qm]), 9))
        assert lev.tolist() == list(range(-(1 << Qm // 2) + 1, 1 << Qm // 2, 2))
        # Gray: the nearest neighbours along an axis differ in one bit, and the demapper's signs on a point are its bits
        order = np.argsort(x.real + 1000 * x.imag, kind="stable")
        row = order[:1 << Qm // 2]
        assert all(bin(int(a) ^ int(b)).count("1") == 1 for a, b in zip(row[:-1], row[1:]))
        assert np.array_equal((F.demap(x, np.ones(x.size), Qm) < 0).astype(np.uint8), F.bits_of(Qm))
    # QPSK b0 b1 = 0 0 is (1 + j) / sqrt 2; 16QAM 0 0 0 0 is (1 + j) / sqrt 10 and 1 0 1 0 is (-3 + j) / sqrt 10 (38.211 5.1.3, 5.1.4)
    assert np.isclose(F.points(2)[0], (1 + 1j) / np.sqrt(2)) and np.isclose(F.points(4)[0], (1 + 1j) / np.sqrt(10))
    assert np.isclose(F.points(4)[0b0101], (-3 + 1j) / np.sqrt(10))
    for cs in (F.coupled_case(2, 3, 0.8, 1), F.coupled_case(4, 2, 0.5, 0, 0.8)):
        a, b = F.ml_exhaustive(cs["rx"], cs["ch"], cs["Qm"], 9), F.ml(cs["rx"], cs["ch"], cs["Qm"], 9, qpsk_interference_weight=1.0)
        assert np.abs(a - b).max() < 1e-9 * np.abs(a).max()
    cs = F.coupled_case(6, 4, 0.8, 1)
    for nvar in F.nvars_of(cs):
        a, b = F.mmse(cs["rx"], cs["ch"], 6, 6, nvar), F.mmse(cs["rx"], cs["ch"], 6, 6, nvar, adjugate=True)
        assert np.abs(a[0] - b[0]).max() < 1e-9 * np.abs(a[0]).max() and np.abs(a[1] - b[1]).max() < 1e-12


# ---- the cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("receiver", RECEIVERS)
def test_cases_satisfy_their_conditions(receiver):
    """On the restatement: nothing saturates or wraps, the level is the formula's, mag_a >= 64 for the MMSE, the columns have the
    correlation the case names, and at the louder level a share of the exact LLRs has the wrong sign."""
    levels = set()
    for cs in cases(receiver):
        h = F._cplx(cs["ch"][:, :, 0])
        corr = abs(np.vdot(h[0], h[1])) / (np.linalg.norm(h[0]) * np.linalg.norm(h[1]))
        assert abs(corr - cs["c"]) < 0.005, (cs["name"], corr)
        assert cs["max_ch"] < 2048                                         # shift_ch_ext = 0 in the two-layer levels
        lv = level_of(receiver, cs)
        levels.add((cs["n_rx"], lv))
        for key, extra in variants(receiver, cs):
            RML.SATURATED.update(adds=0, subs=0)
            planes = []
            got = receiver_llrs(receiver, cs, lv, extra, planes_out=planes)
            assert RML.SATURATED == dict(adds=0, subs=0), key
            assert np.abs(got).max() < 32767, key
            for l in range(1 if receiver == "single" else 2):              # the matched filters' 16-bit sums did not wrap
                rx = cs["rx1"] if receiver == "single" else cs["rx"]
                y = compensate_np(rx, cs["ch"][l], 2, lv)[0].astype(np.float64)
                z = (F._cplx(cs["ch"][l]).conj() * F._cplx(rx)).sum(0) * 2.0 ** -lv
                assert np.abs(y[:, 0] + 1j * y[:, 1] - z).max() < 8 and np.abs(y).max() < 32767, key
            if receiver != "ml":
                assert all(np.abs(p.astype(np.int64)).max() < 32767 for p in planes), key
            if receiver == "mmse":
                assert min(int(p[:, 1].min()) for p in planes) >= 64, key
                E = (np.abs(h) ** 2).sum(1).max() * 2.0 ** -lv + extra[0]   # the diagonal of HhH after the shift, nvar added
                assert E < 32767, key
            want = model_llrs(receiver, cs, lv, extra, **({"qpsk_interference_weight": 1.0} if receiver == "ml" else {}))
            bits = cs["bits"][:, 0] if receiver == "single" else cs["bits"]
            share = float(((want < 0) != bits).mean())
            assert (0.005 < share < 0.45) if cs["loud"] else share < 0.005, (key, share)
    want = {"single": {(2, 10), (3, 10), (4, 11)}, "mmse": {(2, 6), (4, 6)}, "ml": {(2, 9), (3, 9), (4, 9)}}[receiver]
    assert levels == want


# ---- the bound, the restatement and the CPU forms ------------------------------------------------------------------------
@pytest.mark.parametrize("receiver", RECEIVERS)
def test_restatement_and_cpu_forms_within_the_bound(built, receiver):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    dev = deviations(receiver)
    for Qm in sorted({cs["Qm"] for cs in cases(receiver)}):
        worst = max(d for key, d in dev.items() if restated(receiver)[key][0]["Qm"] == Qm)
        measured, bound = F.BOUNDS[(receiver, Qm)]
        print(f"{receiver} Qm {Qm}: restatement's worst deviation {worst:.2f} LSB, table {measured}, bound {bound}")
        assert abs(worst - measured) < 0.006 and bound == math.ceil(1.5 * measured), (receiver, Qm, worst)
    for key, (cs, extra, lv, got) in restated(receiver).items():
        assert dev[key] <= bound_of(receiver, cs), (key, dev[key])
        assert level_of(receiver, cs, m) == lv
        lib = receiver_llrs(receiver, cs, lv, extra, m)
        d = float(np.abs(lib - model_llrs(receiver, cs, lv, extra)).max())
        assert d <= bound_of(receiver, cs), (key, d)
        assert np.array_equal(lib, got), key
    if receiver == "mmse":
        # the equalised point: y / K against xhat, in units of the constellation's spacing
        for key, (cs, extra, lv, got) in restated(receiver).items():
            _, xhat, K = F.mmse(cs["rx"], cs["ch"], cs["Qm"], lv, extra[0])
            at, nb = F.segments_of(cs)[-1]
            y = got[at:at + nb, :, :2].astype(np.float64)
            err = np.abs((y[..., 0] + 1j * y[..., 1]) / K[at:at + nb, None] - xhat[at:at + nb])
            assert err.max() < 0.25 * 2 / np.sqrt(F.NORM[cs["Qm"]]), (key, err.max())


# ---- the misreadings -------------------------------------------------------------------------------------------------------
def _is(**want):
    return lambda cs, extra: all(cs[k] in v for k, v in want.items())


# mutation -> (rule for the cases that notice it, the runs that depart from the rule)
C_POS = (0.5, 0.8, 0.95)
NOTICED = {
    "first_antenna_energy": (_is(Qm=(4, 6, 8)), set()),                                   # QPSK takes no magnitude
    "b_c_exchanged": (_is(c=C_POS), {"Qm8-rx4-c0.5-loud-nvar0", "Qm8-rx4-c0.5-loud-nvar+"}),
    # 2 sigma^2 = 18 is too little against |h|^2 2^-6 = 3000 n_rx, but for one ill-conditioned quiet case
    "nvar_on_one_entry": (lambda cs, extra: cs["loud"] and extra[0] > 0, {"Qm8-rx2-c0.95-quiet-nvar+"}),
    "no_conjugate_in_hh": (lambda cs, extra: True, set()),
    "rho_conjugated": (_is(c=C_POS), set()),
    "rho_exchanged": (_is(c=C_POS), set()),
    "int_mag_from_desired": (lambda cs, extra: cs["name"].endswith(f"l1x{F.LAYER1_SCALE}"), set()),   # equal layers cannot tell
    "a_sq_dropped": (_is(Qm=(4,), c=C_POS), set()),                                       # QPSK: |x|^2 is constant
    "interference_abs_inverted": (_is(Qm=(4,), c=C_POS), set()),
    "mag_class_exchanged": (_is(Qm=(4,)), set()),
    "bits_1_2_exchanged": (_is(Qm=(4,)), set()),
}


@pytest.mark.parametrize("receiver,mut", [(r, mu) for r in RECEIVERS for mu in F.MUTATIONS[r]])
def test_a_misread_model_is_noticed(receiver, mut):
    dev = deviations(receiver, mut=mut)
    noticed = {key for key, d in dev.items() if d > 2 * bound_of(receiver, restated(receiver)[key][0])}
    rule, odd = NOTICED[mut]
    want = {key for key, (cs, extra, lv, got) in restated(receiver).items() if rule(cs, extra)} ^ odd
    print(mut, len(noticed), "of", len(dev), "runs notice it")
    assert noticed, mut
    assert noticed == want, (mut, sorted(noticed - want), sorted(want - noticed))


@pytest.mark.parametrize("receiver", ["mmse", "ml"])
def test_uncorrelated_columns_alone_miss_the_coupling_terms(receiver):
    """With the c = 0 cases alone a receiver that conjugated rho, took the other layer's rho, exchanged B and C, dropped a_sq or
    inverted interference_abs would pass: against the misread model no c = 0 run even leaves the bound.  (The channel of the
    end-to-end tests is orthogonal only up to the spread of its gains; its correlation is printed for the record.)"""
    from test_rx_mmse_host import mmse_e2e_case
    n = 0
    for mut in COUPLING[receiver]:
        dev = deviations(receiver, mut=mut)
        for key, (cs, extra, lv, got) in restated(receiver).items():
            if cs["c"] == 0.0:
                assert dev[key] <= bound_of(receiver, cs), (mut, key, dev[key])
                n += 1
    assert n >= 12 * len(COUPLING[receiver])
    for Qm, n_rx in ((6, 2), (6, 4), (8, 2), (8, 4)):
        h = F._cplx(mmse_e2e_case(Qm, n_rx)[4])
        print(f"end-to-end channel Qm {Qm} n_rx {n_rx}: correlation {abs(np.vdot(h[0], h[1])) / (np.linalg.norm(h[0]) * np.linalg.norm(h[1])):.3f}")


def test_qpsk_detector_is_max_log_only_for_uncorrelated_layers():
    """The reference's QPSK-QPSK detector weights the interference term 1 / sqrt 2 of max-log.  Against the exact
    max-log model the restatement stays inside the bound at c = 0 and leaves it at every c >= 0.5."""
    dev = deviations("ml", qpsk_interference_weight=1.0)
    seen = set()
    for key, (cs, extra, lv, got) in restated("ml").items():
        if cs["Qm"] != 2:
            continue
        seen.add(cs["c"])
        if cs["c"] == 0.0:
            assert dev[key] <= bound_of("ml", cs), (key, dev[key])
        else:
            assert dev[key] > 2 * bound_of("ml", cs), (key, dev[key])
            if cs["loud"]:
                exact = model_llrs("ml", cs, lv, qpsk_interference_weight=1.0)
                assert 0.005 < ((got < 0) != (exact < 0)).mean() < 0.2, key
    assert seen == set(F.CORRELATIONS)
