"""The fast decoder's schedule knobs on the CPU, and the guard over every NRLDPC_HIP_* switch.

1. Every knob value of tests/switch_knobs.py through the emulator (tests/emul: tasks, tickets, pairs and ext_global walked exactly
   as the descriptor lists them), both workgroup shapes, bit-exact against the oracle.
2. Every knob value changes the descriptor of at least one code of the list -- a value that moves nothing tests nothing; the codes
   it moves are what tests/test_gpu_switches.py runs it on.
3. Every switch the library reads (getenv in csrc/) and every switch INTEGRATION section 3c documents is in the table of
   tests/test_gpu_switches.py, with a probe or a one-line exemption, and every switch read is documented.

Says nothing about barriers, LDS capacity, queue draws with odd wave counts or the `fair` turns: tests/test_gpu_switches.py."""
import re
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as O
import switch_knobs as K
from common import kbits, make_llr, random_info

ROOT = Path(__file__).resolve().parent.parent


def emul_decode(fast, BG, Z, R, llr, it, use_crc=False, E=0, init=0x3c):
    L = K.emul_lib()
    out = np.full(68 * 384 + 64, init, np.uint8)
    llr = np.ascontiguousarray(llr, dtype=np.int8)
    L.ldpc_emul_set_fast_shape(K.SHAPES[fast])
    n = L.ldpc_emul_decode_fast(BG, Z, R, it, 0, int(use_crc), E, 1, llr.ctypes.data, out.ctypes.data)
    return n, out[:O.out_bytes(BG, Z, R, 0)]


@pytest.fixture(scope="module")
def cases(built):
    """per code: the inputs (two noisy code words, one uniform int8) and the oracle's results -- computed once, the knobs do not
    enter: [(llr, cap, use_crc, E, (n_iter, out))]"""
    rng = np.random.default_rng(20)
    out = {}
    for BG, Z, R in K.CODES:
        info = random_info(rng, BG, Z, with_crc24b=True)
        Kb = kbits(BG, Z)
        llrs = [make_llr(rng, BG, Z, R, 1.0, info), make_llr(rng, BG, Z, R, -1.0, info), make_llr(rng, BG, Z, R, "rand")]
        runs = [(llr, cap, False, 0) for llr in llrs for cap in (1, 8)]
        assert Kb % 8 == 0 and Kb >= 48
        runs.append((llrs[0], 8, True, Kb))                     # the CRC stop, once per code
        out[(BG, Z, R)] = [(llr, cap, crc, E, O.decode(BG, Z, R, llr, cap, 0, crc, E, 1, out_init=0x3c)) for llr, cap, crc, E in runs]
    return out


def test_the_inputs_stop_in_different_ways(cases):
    """the sweep below sees early stops, capped runs and CRC stops on every code"""
    for code, runs in cases.items():
        its = [ref[0] for _, cap, crc, _, ref in runs if cap == 8 and not crc]
        assert min(its) < 9 and max(its) == 9, (code, its)
        assert runs[-1][2] and 3 <= runs[-1][4][0] < 9, (code, runs[-1][4][0])


@pytest.mark.parametrize("label", list(K.KNOB_VALUES))
def test_knob_value_through_the_emulator(cases, label):
    """ldpc_emul_decode_fast under the knob value, throughput and latency shape, every code of the list: pass count and output
    bytes equal the oracle's.  Where the builder gives the fast section up under a value (f_ok = 0: switch_knobs.FALLS_BACK, nowhere
    else) the emulator refuses, as the library must: it takes such a code off the fast kernel altogether, and the GPU half runs it
    as a "falls back, same results" case."""
    gave_up = set()
    with K.knob_env(K.KNOB_VALUES[label]):
        for (BG, Z, R), runs in cases.items():
            for shape in K.SHAPES:
                if K.fast_info(BG, Z, R, shape)["f_ok"] == 0:
                    gave_up.add((label, (BG, Z, R), shape))
                    assert emul_decode(shape, BG, Z, R, runs[0][0], 8)[0] == -2
                    continue
                for i, (llr, cap, crc, E, ref) in enumerate(runs):
                    n, out = emul_decode(shape, BG, Z, R, llr, cap, crc, E)
                    assert n == ref[0] and np.array_equal(out, ref[1]), (label, BG, Z, R, shape, i, n, ref[0])
    assert gave_up == {f for f in K.FALLS_BACK if f[0] == label}, gave_up


def test_every_knob_value_moves_a_descriptor(built):
    """Each value differs byte-wise from the default on at least one code of the list (otherwise it would be run and prove
    nothing), and the knobs act where the builder's code says they do."""
    aff = K.AFFECTED
    assert aff is K.affected_codes() and set(aff) == set(K.KNOB_VALUES)
    for label, codes in aff.items():
        assert len(codes) >= 1, label
    thr = {label: {c[:3] for c in codes if c[3] == "throughput"} for label, codes in aff.items()}
    lat = {label: {c[:3] for c in codes if c[3] == "latency"} for label, codes in aff.items()}
    for label in aff:
        if label.startswith(("FAST_WAVES", "EXT_GLOBAL")):
            assert thr[label] and not lat[label], label          # the latency shape takes its waves from the task count alone
    assert all(c[0] == 1 for c in thr["PAIR19=0"] | lat["PAIR19=0"]) and thr["PAIR19=0"]        # BG1 has the degree-19 rows
    for label in ("CN_DOUBLE=0", "CN_DOUBLE=3", "CN_DOUBLE=4"):
        assert thr[label] and all(Z >= 256 and R in (13, 15) for _, Z, R in thr[label]), (label, thr[label])
    assert (1, 384, 23) in thr["EXT_GLOBAL=0"]                   # the one code of the list that defaults to ext_global = 1
    assert (1, 384, 13) in thr["EXT_GLOBAL=1"] and (2, 384, 15) in thr["EXT_GLOBAL=1"]
    for w in (5, 7, 9, 13):                                      # wave counts the default search never picks
        with K.knob_env({"FAST_WAVES": str(w)}):
            assert K.fast_info(1, 384, 13)["threads"] == 64 * w
    # what the GPU half reads back through nrLDPC_hip_code_info moves with these four knobs
    with K.knob_env({}):
        d0 = {c: K.fast_info(*c) for c in K.CODES}
    for label, fields in (("FAST_WAVES=5", ("threads",)), ("EXT_GLOBAL=1", ("lds_bytes",)), ("CN_DOUBLE=0", ("cn_tasks",)),
                          ("PAIR19=0", ("cn_tasks",))):
        with K.knob_env(K.KNOB_VALUES[label]):
            moved = [c for c in K.CODES if any(K.fast_info(*c)[f] != d0[c][f] for f in fields)]
        assert moved and set(moved) <= thr[label], (label, moved)


def test_knob_env_restores_the_environment():
    import os
    os.environ["NRLDPC_HIP_BN_GROUP"] = "4"
    try:
        with K.knob_env({"FAST_WAVES": "3"}):
            assert os.environ["NRLDPC_HIP_FAST_WAVES"] == "3" and "NRLDPC_HIP_BN_GROUP" not in os.environ
        assert os.environ["NRLDPC_HIP_BN_GROUP"] == "4" and "NRLDPC_HIP_FAST_WAVES" not in os.environ
    finally:
        del os.environ["NRLDPC_HIP_BN_GROUP"]


# ---- completeness guard ---------------------------------------------------------------------------------------------------
def switches_read_by_the_library():
    names = set()
    for p in sorted((ROOT / "openairinterface5g_amd" / "csrc").iterdir()):
        if p.suffix in (".c", ".cpp", ".h", ".hip"):
            names |= set(re.findall(r'getenv\(\s*(?:S\.role == 1 \? )?"NRLDPC_HIP_([A-Z0-9_]+)"(?:\s*:\s*"NRLDPC_HIP_([A-Z0-9_]+)")?', p.read_text()))
    return {n for pair in names for n in pair if n}


def switches_documented():
    text = (ROOT / "INTEGRATION.md").read_text()
    sec = text[text.index("## 3c. Environment switches"):]
    sec = sec[:sec.index("\n## ", 4)]
    rows = [ln for ln in sec.splitlines() if ln.startswith("| `NRLDPC_HIP_")]
    return {n for ln in rows for n in re.findall(r"`NRLDPC_HIP_([A-Z0-9_]+)", ln.split("|")[1])}


def guard_problems(read, documented, table):
    """what the guard objects to, as a list of strings (empty: all is well)"""
    bad = []
    for n in sorted(read - documented):
        bad.append(f"{n}: read in csrc/ but not in the table of INTEGRATION section 3c")
    for n in sorted((read | documented) - set(table)):
        bad.append(f"{n}: not in SWITCHES of tests/test_gpu_switches.py (a probe or an exemption)")
    for n in sorted(set(table) - (read | documented)):
        bad.append(f"{n}: in SWITCHES but neither read in csrc/ nor documented (misspelt?)")
    return bad


def test_every_switch_is_probed_or_exempted():
    import test_gpu_switches as G
    read, documented = switches_read_by_the_library(), switches_documented()
    assert len(read) >= 50 and {"PAIR19", "ENC_SLOTS", "SRV_SLOTS", "TB_PULL_MAX_MB", "ZC"} <= read, sorted(read)
    assert len(documented) >= 45 and {"T2_LIB", "LIB", "TB_PULL_MAX_MB", "ENC_SLOTS"} <= documented, sorted(documented)
    assert not guard_problems(read, documented, G.SWITCHES), guard_problems(read, documented, G.SWITCHES)
    # the guard notices a name that is taken out of the table, one that is misspelt in it and one that is not documented
    t = dict(G.SWITCHES)
    del t["PAIR19"]
    t["PAIR91"] = ("probe", "x")
    assert len(guard_problems(read, documented, t)) == 2
    assert guard_problems(read, documented - {"TB_PRIO"}, G.SWITCHES) == ["TB_PRIO: read in csrc/ but not in the table of INTEGRATION section 3c"]
    names_in_sets = {k[len(K.PREFIX):] for s in G.SWITCH_SETS for k in s["env"]}
    for name, (kind, what) in G.SWITCHES.items():
        assert kind in ("probe", "exempt") and what, name
        if kind == "probe":                                      # a probed switch is set by at least one switch set
            assert name in names_in_sets, name
            assert all(p in G.PROBES for p in what.split(",")), (name, what)
            assert any(K.PREFIX + name in s["env"] and set(what.split(",")) & set(s["probes"]) for s in G.SWITCH_SETS), name
        else:
            assert name not in names_in_sets, name
    for s in G.SWITCH_SETS:                                      # ... and a set only sets switches the table knows as probed
        for k in s["env"]:
            assert k.startswith(K.PREFIX) and G.SWITCHES[k[len(K.PREFIX):]][0] == "probe", (s["id"], k)
        assert s["probes"] and all(p in G.PROBES for p in s["probes"]), s["id"]


def test_a_fall_back_value_runs_every_probe_the_table_names(built):
    """the guard accepts any value of a name; a value under which the builder gives a shape up (switch_knobs.FALLS_BACK) must be in a
    set that runs ALL the probes SWITCHES names for that knob, and that set must claim the fall-back as evidence"""
    import test_gpu_switches as G
    assert K.FALLS_BACK
    for label, code, _ in K.FALLS_BACK:
        (name, value), = K.KNOB_VALUES[label].items()
        sets = [s for s in G.SWITCH_SETS if s["env"].get(K.PREFIX + name) == value]
        assert sets, label
        for s in sets:
            assert set(G.SWITCHES[name][1].split(",")) <= set(s["probes"]), (label, s["id"])
            assert ("falls_back", "fast", code) in s["evidence"], (label, s["id"])
            knobs = {k[len(K.PREFIX):]: v for k, v in s["env"].items() if k[len(K.PREFIX):] in K.KNOBS}
            with K.knob_env(knobs):                      # ... and the set's other knobs leave the fall-back in place
                assert not (K.fast_info(*code, "throughput")["f_ok"] and K.fast_info(*code, "latency")["f_ok"]), s["id"]


def test_switch_set_evidence_is_something_the_set_moves(built):
    """every ("code_info", field, code) a switch set names as evidence differs, in the table builder, between the default
    configuration and the set's knobs -- otherwise the child's assertion could not hold (or would hold for no reason)"""
    import test_gpu_switches as G
    with K.knob_env({}):
        d0 = {c: K.fast_info(*c) for c in K.CODES}
    for s in G.SWITCH_SETS:
        knobs = {k[len(K.PREFIX):]: v for k, v in s["env"].items() if k[len(K.PREFIX):] in K.KNOBS}
        ev = [e for e in s["evidence"] if e[0] == "code_info"]
        assert ev or not knobs, s["id"]
        with K.knob_env(knobs):
            for _, field, code in ev:
                assert field in G.INFO_INDEX and tuple(code) in K.CODES, (s["id"], field, code)
                assert K.fast_info(*code)[field] != d0[tuple(code)][field], (s["id"], field, code)
                assert K.fast_info(*code, "latency")["f_ok"] and K.fast_info(*code)["f_ok"], (s["id"], code)


def test_every_knob_value_is_in_a_switch_set():
    """part A's values all occur in the GPU half's table, as do the group-2 and group-3 switches of the issue"""
    import test_gpu_switches as G
    have = {(k[len(K.PREFIX):], v) for s in G.SWITCH_SETS for k, v in s["env"].items()}
    for label, short in K.KNOB_VALUES.items():
        if label != "combined":
            assert set(short.items()) <= have, label
    assert any(all(s["env"].get(K.PREFIX + k) == v for k, v in K.KNOB_VALUES["combined"].items()) for s in G.SWITCH_SETS)
    for want in (("SRV_BAR", "0"), ("HOST_PULL", "0"), ("TB_PULL", "0"), ("TB_PULL_MAX_MB", None), ("TB_HOST_CHUNKS", None),
                 ("HOST_CHUNK", None), ("TB_LROW", "0"), ("CUT", "0"), ("MULTI", "0"), ("MULTI", None), ("TB_CRC_CHUNK", "1"),
                 ("TB_CRC_CHUNK", "2"), ("BOUNCE_THREADS", "0"), ("FAIR", "0"), ("TB_FAIR", "0"), ("TB_PRIO", None),
                 ("TB_OVERLAP", "1"), ("TB_STAGGER_US", None), ("PULL_STAGGER_US", "0")):
        assert any(n == want[0] and (want[1] is None or v == want[1]) for n, v in have), want
    assert any(n == "MULTI" and v not in ("0",) for n, v in have)
