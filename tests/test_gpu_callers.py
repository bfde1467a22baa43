"""The DEVICE mem calls as a gNB's worker threads make them: from several threads at once, each on its own stream; on two streams
of one thread with work still pending; from threads that end while their work is still queued; and the three newer uploading calls
back to back with their HOST forms in one thread's contexts.  What is exercised is the state the library keeps per thread behind
the caller's back -- the page-locked descriptor staging area of a TbCtx (DeviceCall::upload and the chain's two upload sites),
its pooled life beyond the thread, the shared scratch and plans -- and the process-wide delay tables.  Every expectation comes from
the CPU forms and restatements (callers_np.py) and is computed single-threaded before any thread starts; outputs are compared for
equality on canary-filled arrays.

The delayed stream.  delay() queues torch.cuda._sleep for a given time, bounded: the sleep kernel's tick rate is measured once.
An event recorded behind the first call on the delayed stream must still be incomplete at the checkpoints (query() is False);
if it is not, the delay was too short, the hazard window never opened and the test FAILS.  Calls that pass through one context back
to back follow callers_np.py's rule for variants, so that a missed ordering shows as wrong values and never as a fault."""
import threading
import time

import numpy as np
import pytest

import callers_np as K
import ul_slot_np as U

pytestmark = pytest.mark.gpu

RB = (2, 3, 5, 8)                 # PRBs of the four threads' slots: table sizes differ per thread
DELAY2_MS = 20.0                  # sized in test_two_streams_of_one_thread_with_work_pending
DELAY3_MS = 80.0                  # sized in test_thread_generations_on_one_delayed_stream
_ticks_per_ms = []


def sleep_rate():
    """ticks of torch.cuda._sleep per millisecond, measured once (and outside anything a test times)"""
    import torch
    if not _ticks_per_ms:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000)                                       # (the kernel's first launch)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(1000000)
        b.record()
        b.synchronize()
        _ticks_per_ms.append(1000000 / a.elapsed_time(b))
    return _ticks_per_ms[0]


def delay(stream, ms):
    """ms milliseconds of torch.cuda._sleep at the tail of `stream`; at most 0.2 s per use"""
    import torch
    assert 0 < ms <= 200
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(ms * sleep_rate()))


def assert_variants_differ(name, calls):
    """a swap of two consecutive calls' descriptors must be visible: their expectations differ in most entries (bit-valued outputs:
    in 40 %, two strings of independent bits agreeing in half their places)"""
    for k in range(len(calls) - 1):
        assert K.differs(calls[k], calls[k + 1]) > K.MOST.get(name, 0.5), (name, k, K.differs(calls[k], calls[k + 1]))


# ---- 1. four threads at once, each on its own stream -----------------------------------------------------------------------------
def test_concurrent_threads_on_their_own_streams(hip):
    """Four threads behind a barrier, each with its own stream (passed as stream=), device tensors, seed and rb_size (2, 3, 5, 8 PRBs
    over 14 symbols on a 1024-point grid, the allocation wrapping round the grid's end), three rounds each with one synchronisation of
    the thread's stream per round.  Threads 0 and 1: one layer, pusch_channel_estimation -> ulsch_channel_level_grid ->
    ulsch_channel_compensation_grid -> ulsch_decode_symbols_device on slot_case's grid.  Threads 2 and 3: two layers on a slot of
    ul_slot_np.py, pusch_channel_estimation (both layers' descriptors) -> ulsch_channel_level_grid_mmse -> ulsch_mmse_2layers_grid ->
    ulsch_decode_symbols_device.  Every thread then: dlsch_encode_symbols_device -> pdsch_resource_mapping_precoded.  Compared per
    round: estimates, level, records, payload (where the oracle ACKs: the two-layer slots), ACK, pass count, soft buffers, layer
    planes, transmit grid."""
    import torch
    m = hip.ldpc
    # fft_size 1024: no GPU test before this one estimates at it, so the four threads' first estimation calls race for the size's
    # delay table in che_table_device.  That property is lost if an earlier test of a session starts to use 1024.
    ul = [K.ul1_chain_call(m, 1024, RB[0]), K.ul1_chain_call(m, 1024, RB[1]), K.ul2_chain_call(m, K.ul2_slot(m, 1024, RB[2], 102)),
          K.ul2_chain_call(m, K.ul2_slot(m, 1024, RB[3], 103, U.T1I))]
    dl = [K.dl_chain_call(m, K.dl_slot(m, 1024, rb, 100 + k)) for k, rb in enumerate(RB)]
    assert all(c.want["ack"][0] == 1 and "pay" in c.want for c in ul[2:]), "the two-layer slots decode"
    streams = [torch.cuda.Stream() for _ in RB]
    torch.cuda.synchronize()
    barrier = threading.Barrier(len(RB))
    errors, took = [], {}

    def worker(k):
        try:
            s = streams[k]
            barrier.wait(timeout=60)
            with torch.cuda.stream(s):
                for rnd in range(3):
                    t0 = time.perf_counter()
                    ul[k].stage()
                    dl[k].stage()
                    ul[k].issue(s.cuda_stream)
                    dl[k].issue(s.cuda_stream)
                    s.synchronize()
                    took[(k, rnd)] = round(time.perf_counter() - t0, 3)
                    errors.extend(ul[k].mismatches((k, rnd, "ul")) + dl[k].mismatches((k, rnd, "dl")))
        except Exception as e:  # noqa: BLE001
            errors.append((k, repr(e)))

    th = [threading.Thread(target=worker, args=(k,)) for k in range(len(RB))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    print("concurrent threads: seconds per (thread, round) from staging to the stream's synchronisation:", sorted(took.items()))
    assert not errors, errors


# ---- 2. one thread, two streams, work pending --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pusch_channel_estimation", "pdsch_resource_mapping_precoded", "ulsch_mmse_2layers_grid", "dlsch_encode_symbols_device",
                                  "ulsch_decode_symbols_device", "cached_plan_encode"])
def test_two_streams_of_one_thread_with_work_pending(hip, name):
    """Stream A carries the delay.  Call 1 on A, an event behind it (checkpoint: not complete), then the same entry point with other
    values on B, on A and on B, one synchronisation at the end: all four outputs are right.  The slot-level calls go through
    DeviceCall::upload, the symbol calls through the chain's TX and RX upload sites and the shared scratch; cached_plan_encode is the
    third call of a PreparedTbBatch, which uploads nothing and shares one plan among the four batches.

    This pins what tb_begin's serialisation buys -- a call on another stream than the thread's last waits for that stream -- and
    cannot prove that guard necessary: without it tb_wait_upload still waits for the previous upload, which closes most of the
    window (what remains is the device job area and the scratch, rewritten on B while A's kernels have yet to read them).

    Host time from queueing the delay to the checkpoint, measured on the MI355X with time.perf_counter: 0.05 ms (cached plan) to
    0.23 ms (precoded mapping) over the six entry points in two sessions.  Ten times the largest is 2.3 ms; DELAY2_MS is 20 ms,
    which also covers a host thread that loses its core for a few milliseconds."""
    import torch
    m = hip.ldpc
    calls = K.BUILDERS[name](m, 4)
    assert_variants_differ(name, calls)
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    order = (A, B, A, B)
    # first use (code objects, buffers, plans' slots) outside the delay: calls 0 and 1 once, then everything staged afresh
    for c, s in zip(calls, order):
        c.stage(s.cuda_stream)
    torch.cuda.synchronize()
    calls[0].issue(A.cuda_stream)
    calls[1].issue(B.cuda_stream)
    torch.cuda.synchronize()
    for c, s in zip(calls, order):
        c.stage(s.cuda_stream)
    ev = torch.cuda.Event()
    sleep_rate()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    delay(A, DELAY2_MS)
    calls[0].issue(A.cuda_stream)
    ev.record(A)
    pending = not ev.query()
    host_ms = (time.perf_counter() - t0) * 1e3
    for c, s in zip(calls[1:], order[1:]):
        c.issue(s.cuda_stream)
    torch.cuda.synchronize()
    print("two streams, %s: %.3f ms of host time before the checkpoint, delay %.0f ms" % (name, host_ms, DELAY2_MS))
    assert pending, "call 1 had run before call 2 was made: the delay (%.0f ms) is too short for %.3f ms of host work" % (DELAY2_MS, host_ms)
    bad = sum((c.mismatches(k) for k, c in enumerate(calls)), [])
    assert not bad, bad


# ---- 3. thread generations on one delayed stream ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pusch_channel_estimation", "pdsch_resource_mapping_precoded", "dlsch_encode_device", "ulsch_decode_device"])
def test_thread_generations_on_one_delayed_stream(hip, name):
    """Four short-lived threads one after the other, each joined before the next starts, each issuing one DEVICE mem call of the same
    entry point on stream S -- its own values, its own output -- behind a delay, and ending while the call is still queued.  One
    synchronisation at the end; output k must equal expectation k.  One entry point per upload site: DeviceCall::upload (estimation,
    precoded mapping), the chain's TX site (dlsch_encode_device, rv 0..3) and its RX site (ulsch_decode_device, rv 0..3).

    A TbCtx outlives its thread: ~CtxHolder drains it and returns it to a LIFO pool, so each generation takes over its predecessor's
    context (if the pool hands out another one, the test passes legitimately) with last == S.  TbCtx::drain() once cleared `pending`
    without waiting for the upload on the caller's stream: the next generation then found nothing to wait for and rewrote the
    page-locked staging area before the queued copy had read it.  drain() now waits for the upload event.

    The checkpoint, after every join: the event recorded behind the first generation's call is not complete, so every generation
    was issued, and every generation's thread ended, with all the calls before it still queued.  Also, as each generation's last
    statement: its own event is not complete.  A thread's exit now waits for its upload, which lies behind the delay; join() returns
    before the thread's C++ thread-local destructors run, so that wait goes on beside the generations that follow (they take another
    context from the pool meanwhile: with the wait in place there is nothing to inherit before the upload has gone).  Under a join()
    that waited for the destructors, the checkpoint could hold only for a library without the wait.

    Host time from queueing the delay to the last join (four thread starts, calls, events and joins), measured on the MI355X with
    time.perf_counter: 1.3 to 4.7 ms over the four entry points in two sessions.  Ten times the largest is 47 ms; DELAY3_MS is 80 ms,
    once per test.

    The parent commit's library on the same machine, same test: no fault, wrong values.  Estimation and precoded mapping:
    generations 0, 1 and 2 wrong, 3 right; the two chain calls: generations 1 and 2 wrong, 0 and 3 right (generation 0 finds the
    plan the warm-up thread left and uploads nothing) -- every queued copy read the staging area as the last generation left it.  The
    runtime reads a page-locked source when the copy executes, not when it is queued."""
    import torch
    m = hip.ldpc
    calls = K.BUILDERS[name](m, 4)
    assert_variants_differ(name, calls)
    S = torch.cuda.Stream()
    errors = []

    def in_thread(fn, *args):
        def body():
            try:
                fn(*args)
            except Exception as e:  # noqa: BLE001
                errors.append(repr(e))
        t = threading.Thread(target=body)
        t.start()
        t.join()

    # first use outside the delays, in a thread of its own: the pool then holds a context with its stream, event and buffers
    calls[0].stage(S.cuda_stream)
    torch.cuda.synchronize()
    in_thread(calls[0].issue, S.cuda_stream)
    torch.cuda.synchronize()
    for c in calls:
        c.stage(S.cuda_stream)
    sleep_rate()
    torch.cuda.synchronize()
    events, queued, after_join = [], [], []

    def generation(k):
        calls[k].issue(S.cuda_stream)
        ev = torch.cuda.Event()
        ev.record(S)
        events.append(ev)
        queued.append(not ev.query())

    t0 = time.perf_counter()
    delay(S, DELAY3_MS)
    for k in range(4):
        in_thread(generation, k)
        after_join.append(bool(events) and not events[0].query())
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    print("generations, %s: %.3f ms of host time from the delay to the last join, delay %.0f ms" % (name, host_ms, DELAY3_MS))
    assert not errors, errors
    assert queued == [True] * 4 and after_join == [True] * 4, ("the first call had run before the last generation ended: the delay (%.0f ms) is too short "
                                                                "for %.3f ms of host work" % (DELAY3_MS, host_ms), queued, after_join)
    bad = sum((c.mismatches(k) for k, c in enumerate(calls)), [])
    assert not bad, bad


# ---- 4. the three newer uploaders in one thread's contexts -------------------------------------------------------------------------
def test_newer_uploaders_share_one_threads_contexts(hip):
    """test_calls_share_one_threads_contexts of test_gpu_slot_calls.py for pdsch_resource_mapping_precoded,
    ulsch_channel_level_grid_mmse and ulsch_mmse_2layers_grid: each call HOST then DEVICE, back to back on one thread with one
    synchronisation at the end; a small slot, a large one whose staged inputs outgrow what the small one left, the small one again."""
    import torch
    m = hip.ldpc
    small = (K.dl_slot(m, 128, 2, 81), K.ul2_slot(m, 128, 4, 82))
    large = (K.dl_slot(m, 2048, 106, 83), K.ul2_slot(m, 2048, 106, 84))
    # The staging buffers grow to 1.5 x the request + 4096 bytes (ThreadCtx::ensure).  A HOST call of the small round stages at most its
    # arrays -- grid and estimates, or layer planes and transmit grid -- and its tables (below 8 KiB): less than 64 KiB, so the round
    # leaves at most 1.5 x 65536 + 4096 bytes.  Every HOST call of the large round stages at least the layer entries it reads (the
    # mapping) or three planes of estimates (the MMSE calls: the pairs' range, (2 n_rx - 1) strides and the allocation): more than that.
    for d, sl in (small,):
        assert max(sl["rx"].nbytes + sl["ch"].nbytes, d["lay"].nbytes + d["tx"].nbytes) + 8192 < 65536
    for d, sl in (large,):
        assert min(4 * 2 * d["S"], 4 * 3 * sl["ch_stride"]) > 1.5 * 65536 + 4096
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for rnd, (d, sl) in enumerate((small, large, small)):
        dc = [K.map_call(m, d), K.level_mmse_call(m, sl), K.mmse_call(m, sl)]
        host = {}
        with torch.cuda.stream(side):
            for c in dc:
                c.stage()
            for c, host_form, arg in zip(dc, (K.map_host, K.level_mmse_host, K.mmse_host), (d, sl, sl)):
                host.update(host_form(m, arg))
                c.issue(side.cuda_stream)
        torch.cuda.synchronize()
        bad = sum((c.mismatches((rnd, "device")) for c in dc), [])
        for c in dc:
            for k, w in c.want.items():
                if not np.array_equal(host[k].reshape(-1), w.reshape(-1)):
                    bad.append((rnd, "host", k, np.flatnonzero(host[k].reshape(-1) != w.reshape(-1))[:6].tolist()))
        assert not bad, bad
