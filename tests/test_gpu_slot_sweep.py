"""The slot-level calls on the GPU over the seeded random draws of slot_sweep_np.py.  The seeds are a prefix of those of
test_slot_sweep_host.py, so every draw has already run in bounds through the emulated kernels on the CPU; the draws are valid only,
no test provokes a refusal.  Three parts:

  - one test per draw kind, DEVICE mem, against the host forms: the output arrays with slot_sweep_np.MARGIN canary elements on
    either side, equality bit for bit over the whole arrays (delays, peaks, levels, max_ch and nvar too) -- the delay search's
    kind (a) draws, where near-ties and exact ties decide the position, are among them;
  - one drawn sequence of calls of every kind, queued on one side stream with nothing between them and one synchronisation at the
    end, each call with arrays of its own -- a job-area upload or a level / _meas state block that is not ordered behind the
    previous call's kernels would show here -- and the same sequence once more from a second thread on a stream of its own;
  - HOST mem for three seeds per kind: the draws with the most descriptors, which lie far apart and out of order (the staged-span
    arithmetic).

Measured on the MI355X: every DEVICE mem test 0.03 - 0.2 s (chest, 120 draws, is the longest; whichever test runs first also
carries the library's first use, 12 s), the queued sequence of 42 calls run twice 0.04 s, every HOST mem test below 0.05 s; the
file 14 s (measured with 12 delay draws; with the 24 there are now none of the file's tests is among the suite's 15 slowest, the
last of which takes 6.7 s)."""
import threading
import time

import numpy as np
import pytest

import slot_sweep_np as S
from test_slot_sweep_host import COUNTS, same_bits

pytestmark = pytest.mark.gpu

# kind -> seeds 0 .. n - 1 of the DEVICE mem test
GPU_SEEDS = {"front": 40, "grid": 40, "mmse": 30, "ml": 30, "chest": 120, "chest_meas": 40, "time_avg": 60, "delay": 24, "pdsch_map": 80, "pdsch_precoded": 80}
SEQ_ROUNDS = 3                                                         # rounds over the ten kinds, a seed each: 14 calls a round
JOIN_S = 120
_cache = {}


def drawn(m, call, seed):
    """the draw and what the host forms make of it, computed once per session"""
    if (call, seed) not in _cache:
        d = S.draw(call, seed)
        _cache[(call, seed)] = (d, S.expected(m, d))
    return _cache[(call, seed)]


def staged(d):
    """the draw's inputs and canary-filled output arrays as device tensors (on the current stream)"""
    import torch
    ins = {k: None if v is None else torch.from_numpy(np.array(v)).cuda() for k, v in d["inputs"].items()}
    full = {k: torch.from_numpy(v).cuda() for k, v in S.fresh_outputs(d).items()}
    outs = {k: v[S.MARGIN * d["outputs"][k][2]:] for k, v in full.items()}
    return ins, full, outs


def mismatches(d, want, got):
    return [(d["call"], d["seed"], k, (np.flatnonzero(got[k] != w)[:6] - S.MARGIN * d["outputs"][k][2]).tolist()) for k, w in want.items()
            if not same_bits(got[k], w)]


@pytest.mark.parametrize("call", list(GPU_SEEDS))
def test_device_mode_equals_the_host_form(hip, call):
    import torch
    m = hip.ldpc
    assert GPU_SEEDS[call] <= COUNTS[call]
    if call == "delay":                                                # the running maximum over equal antennas: exact ties on the device
        assert sum("tie_running_max" in S.draw(call, seed)["seams"] for seed in range(GPU_SEEDS[call])) >= 3
    t0, bad = time.time(), []
    for seed in range(GPU_SEEDS[call]):
        d, want = drawn(m, call, seed)
        ins, full, outs = staged(d)
        S.run(m, d, ins, outs)
        torch.cuda.synchronize()
        bad += mismatches(d, want, {k: v.cpu().numpy() for k, v in full.items()})
        assert all(v is None or np.array_equal(ins[k].cpu().numpy(), v) for k, v in d["inputs"].items()), (call, seed, "an input changed")
    print(f"\n{call}: {GPU_SEEDS[call]} draws in DEVICE mem, {time.time() - t0:.1f} s")
    assert not bad, bad[:8]


def sequence(m):
    """[(draw, expectation)]: SEQ_ROUNDS rounds over the kinds, more until every fft_size has appeared"""
    seq, sizes, rnd = [], set(), 0
    while rnd < SEQ_ROUNDS or sizes != set(S.SIZES):
        assert rnd < min(GPU_SEEDS.values()), "the sequence stays inside the seeds the per-kind tests have run"
        for call in S.CALLS:
            seq.append(drawn(m, call, rnd))
            sizes |= {s["fft_size"] for s in seq[-1][0]["segs"] if "fft_size" in s}
        rnd += 1
    return seq


def queue_and_compare(m, seq, stream, errors):
    """everything staged first; then every call queued on `stream` with nothing in between; one synchronisation; every output"""
    import torch
    try:
        with torch.cuda.stream(stream):
            st = [staged(d) for d, _ in seq]
            stream.synchronize()
            for (d, _), (ins, full, outs) in zip(seq, st):
                S.run(m, d, ins, outs)
            stream.synchronize()
        for (d, want), (ins, full, outs) in zip(seq, st):
            errors += mismatches(d, want, {k: v.cpu().numpy() for k, v in full.items()})
    except Exception as e:  # noqa: BLE001
        errors.append(repr(e))


def test_a_drawn_sequence_on_one_stream_and_again_from_a_second_thread(hip):
    import torch
    m = hip.ldpc
    seq = sequence(m)
    kinds = [d["call"] for d, _ in seq]
    n_calls = sum(2 if k in ("front", "grid", "mmse", "ml") else 1 for k in kinds)      # those four are a level and a receiver call
    assert n_calls >= 40 and all(kinds.count(k) >= 2 for k in S.CALLS) and all(a != b for a, b in zip(kinds, kinds[1:]))
    assert {s["fft_size"] for d, _ in seq for s in d["segs"] if "fft_size" in s} == set(S.SIZES)
    t0, errors = time.time(), []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    queue_and_compare(m, seq, side, errors)
    assert not errors, errors[:8]
    other = torch.cuda.Stream()
    th = threading.Thread(target=queue_and_compare, args=(m, seq, other, errors))
    th.start()
    th.join(JOIN_S)
    assert not th.is_alive(), "the second thread's sequence did not finish"
    print(f"\nsequence: {len(seq)} draws, {n_calls} calls, twice, {time.time() - t0:.1f} s")
    assert not errors, errors[:8]


def host_seeds(call):
    """the three draws of the GPU prefix with the most descriptors: the widest spans, shuffled"""
    n = {seed: len(S.draw(call, seed)["segs"]) for seed in range(min(GPU_SEEDS[call], 30))}
    return sorted(sorted(n, key=lambda seed: (-n[seed], seed))[:3])


@pytest.mark.parametrize("call", list(GPU_SEEDS))
def test_host_mode_equals_the_host_form(hip, call):
    m = hip.ldpc
    for seed in host_seeds(call):
        d, want = drawn(m, call, seed)
        assert len(d["segs"]) >= 2, (call, seed)
        full = S.fresh_outputs(d)
        S.run(m, d, d["inputs"], {k: S.inner(v, d["outputs"][k][2]) for k, v in full.items()})
        bad = mismatches(d, want, full)
        assert not bad, bad
