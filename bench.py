#!/usr/bin/env python3
"""bench.py -- BASELINE.json's metric on BASELINE.json's configuration.

metric   : coded Gb/s of the NR LDPC decoder, BG1 Zc=384 R=1/3, 8-iteration cap (configs[1]): batch of 1024
           code blocks per GPU and step, inputs resident in HBM before the timed region starts.
step     : one decode of the whole batch through LDPCdecoder_batch (C ABI, device pointers).
clocks   : the GPU's clocks ramp for ~30 ms of continuous work after idling (profiles/r06/clock_ramp.txt).  The W + K steps are
           taken twice: straight after set-up ("after_idle", what rounds 1-5 called value) and again after untimed launches
           have brought the clocks up (value).  Both timed regions are exactly K full steps.
value    : ranks * steps * 1024 * 25 344 coded bits / wall time (max over ranks), FIXED-WORK regime: the LLRs are
           a code word buried in noise (Es/N0 = -12 dB) so the parity check never passes and all 9 CN/BN passes
           run for every block -- the worst case the 8-iteration cap allows.  An operating-point run (early
           stop active, BLER and mean pass count reported) is added under "operating_point".
scaling  : weak -- every rank decodes its own 1024 blocks; code blocks are independent, there is no
           collective on the data path (results are gathered once, outside the timed region).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

BG, Z, R, MAX_ITER, BATCH = 1, 384, 13, 8, 1024
K = 22 * Z
N_TX = 66 * Z              # coded bits per block at the mother rate
NUM_LLR = 68 * Z
EDGES = 316
PASSES_FIXED = MAX_ITER + 1
A_MIN = NUM_LLR + K // 8                                   # compulsory HBM bytes per block (27 168)
STRONG_DEADLINE_S = int(os.environ.get("BENCH_DEADLINE_S", "120"))   # secondary legs at N > 1: see main()
A_MSG = A_MIN + PASSES_FIXED * 4 * EDGES * Z               # reference dataflow bytes per block (4 395 552)
HBM_PEAK_GBS = 8000.0                                      # MI355X_MICROARCH.md: 8 TB/s spec


def make_batch(pkg, torch, snr_db, seed):
    """Random info bits -> product encoder (GPU) -> BPSK + AWGN -> ldpctest's quantiser (coding_unitary_defs.h:37-49)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    info = torch.randint(0, 256, (BATCH, K // 8), dtype=torch.uint8, device="cuda", generator=g)
    coded = torch.empty((BATCH, N_TX), dtype=torch.uint8, device="cuda")
    pkg.encode_batch_device(BG, Z, info, coded)
    sigma = 1.0 / np.sqrt(2.0 * 10.0 ** (snr_db / 10.0))
    y = 1.0 - 2.0 * coded.float() + sigma * torch.randn((BATCH, N_TX), device="cuda", generator=g)
    llr = torch.zeros((BATCH, NUM_LLR), dtype=torch.int8, device="cuda")
    llr[:, 2 * Z:] = torch.clamp(torch.floor(y / (sigma / 16.0)), -128, 127).to(torch.int8)
    torch.cuda.synchronize()
    return info, llr


def usable_cores():
    """Threads the CPU baseline may really use: the affinity mask capped by the cgroup CPU quota (a GPU box leases a
    slice of a 256-thread host: round 1 printed the mask size and understated the per-core rate ~30x)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        q, per = Path("/sys/fs/cgroup/cpu.max").read_text().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except Exception:
        try:
            q = int(Path("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read_text())
            per = int(Path("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read_text())
            if q > 0:
                quota = q / per
        except Exception:
            pass
    threads = n if quota is None else max(1, min(n, int(quota + 0.5)))
    return threads, n, quota


def cpu_baseline(llr_host):
    """The oracle's vectorisable restatement of the reference decoder (oracle/oracle_ldpc_decoder_vec.c: plain C that
    gcc vectorises, AVX-512BW / AVX2 / baseline clones, bit-identical to the scalar restatement) timed on this box's
    host cores on a bounded sample of the same fixed-work batch: one pthread per usable core, block b on thread
    b % threads -- the reference's own parallelisation (one thread-pool job per segment).  A reported baseline, not the
    target.  `cores` = threads that ran (affinity mask capped by the cgroup quota); `cores_effective` = multi-thread rate
    / single-thread rate, i.e. what the lease really delivered."""
    sys.path.insert(0, str(ROOT / "tests"))
    import oracle_lib as O
    O.lib()
    threads, mask, quota = usable_cores()
    threads = min(threads, 64)
    n1 = 3000
    llr1 = llr_host[np.arange(n1) % llr_host.shape[0]]
    O.decode_mt(1, BG, Z, R, llr1[:8], MAX_ITER, vec=True)          # page in
    t1 = time.perf_counter()
    its1, _ = O.decode_mt(1, BG, Z, R, llr1, MAX_ITER, vec=True)
    dt1 = time.perf_counter() - t1
    single = n1 * N_TX / dt1 / 1e9
    per_thread = max(200, int(12.0 / (dt1 / n1) / 1))               # ~12 s of work per thread
    per_thread = min(per_thread, 60000)
    blocks = threads * per_thread
    llr = llr_host[np.arange(blocks) % llr_host.shape[0]]
    O.decode_mt(threads, BG, Z, R, llr[:threads], MAX_ITER, vec=True)   # warm the threads
    t0 = time.perf_counter()
    its, _ = O.decode_mt(threads, BG, Z, R, llr, MAX_ITER, vec=True)
    dt = time.perf_counter() - t0
    value = blocks * N_TX / dt / 1e9
    return {"value": value, "unit": "Gb/s", "cores": threads, "kind": "port",
            "cores_effective": value / single, "single_core_value": single,
            "affinity_mask_cpus": mask, "cgroup_cpu_quota": quota,
            "reference_measured": {"value_per_core": [0.074, 0.094], "unit": "Gb/s",
                                   "what": "OAI's own AVX-512 nrLDPC_decoder, same code and 9-pass input, 1 thread "
                                           "(271-343 us per block); 8 threads: 0.46-0.57 Gb/s",
                                   "provenance": "BASELINE.md section 2: survey container (Xeon 2.1 GHz, 8 vCPU), reference "
                                                 "built with a SIMDE->native shim that cannot be rebuilt from this "
                                                 "repository -- not measured on this box"},
            "sample": f"{blocks} blocks of the fixed-work batch ({per_thread} per pthread, {threads} pthreads, "
                      f"mean passes {float(its.mean()):.2f}) in {dt:.2f} s; vectorised C port of the reference "
                      f"decoder (oracle/oracle_ldpc_decoder_vec.c, gcc -O3, runtime-dispatched AVX-512BW/AVX2); "
                      f"1 thread: {n1} blocks in {dt1:.2f} s"}


def strong_slot(pkg, torch, dist, world, rank, steps):
    """BASELINE configs[4]: ONE slot's 64 PUSCH transport blocks (273 PRB x 13 symbols, 64QAM: 1664 code segments) land
    on rank 0 and are decoded by all ranks' GPUs -- LLR ranges scattered point-to-point, the UL-SCH chain per rank on
    whole transport blocks, payloads / ACKs gathered (openairinterface5g_amd/parallel.py ShardedUlsch).  Timed end to
    end on the root, strong scaling (fixed total work).  At N = 1 the same call runs without any exchange."""
    from openairinterface5g_amd import parallel
    m = pkg.ldpc
    A = 213176
    while m.nr_segmentation(A + 24, 1) is None:
        A += 8
    G = (12 * 13 - 6) * 273 * 6
    n_tb = 64
    tbs = [dict(A=A, G=G, BG=1, Qm=6, Nl=1, rv=0, tbslbrm=0, round=0) for _ in range(n_tb)]
    po, co, ho, segs = m.tb_layout(tbs)
    dev = torch.device("cuda", torch.cuda.current_device())
    llr = payload = None
    if rank == 0:
        g = torch.Generator(device="cuda").manual_seed(4242)
        payload = torch.randint(0, 256, (int(po[-1]),), dtype=torch.uint8, device=dev, generator=g)
        coded = torch.zeros(int(co[-1]), dtype=torch.uint8, device=dev)
        m.dlsch_encode_device(tbs, payload, coded)
        llr = ((1.0 - 2.0 * coded.float()) * 10 + 1.8 * torch.randn(coded.numel(), device=dev, generator=g)).round() \
            .clamp(-127, 127).to(torch.int16)
        torch.cuda.synchronize()
    # a process group of ONE rank (BENCH_FORCE_DIST=1 on a one-GPU box): the slot is cut for 4 virtual ranks and the virtual
    # peers' LLRs and results go through real RCCL send / receive pairs to this rank itself (parallel.ShardedUlsch
    # loopback) -- the N > 1 protocol on hardware, not a measurement of N > 1
    loop = int(os.environ.get("BENCH_LOOPBACK_RANKS", "4")) if (dist is not None and world == 1) else 0
    sh = parallel.ShardedUlsch(tbs, device=dev, numMaxIter=MAX_ITER, loopback=loop)
    if dist is not None:
        # every rank reached the collective section with its inputs built (a rank that raised above never gets here and
        # the others find out from the watchdog time-out of this all-reduce instead of hanging in the scatter)
        ready = torch.ones(1, dtype=torch.int32, device=dev)
        dist.all_reduce(ready)
        if int(ready.item()) != world:
            raise RuntimeError("not every rank finished the set-up of the strong-scaling slot")
    for _ in range(2):
        out = sh.decode(llr)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
        torch.cuda.synchronize()
    # (a) the slot as a latency: one slot, wait, next slot -- the host's synchronize() per step is inside the figure;
    t0 = time.perf_counter()
    for _ in range(steps):
        out = sh.decode(llr)
        torch.cuda.synchronize()
    dt_each = time.perf_counter() - t0
    # (b) the slots back to back: K slots enqueued, ONE pair of events on the stream the chain runs on around them (what a
    # profile of the kernels shows; the driver's clock around (a) reads 10 % longer than the kernels take)
    if dist is not None:
        dist.barrier()
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        out = sh.decode(llr)
    e1.record()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ev_ms = e0.elapsed_time(e1)
    share_ms = [dt / steps * 1e3]
    if dist is not None:
        t = torch.tensor([dt, dt_each], dtype=torch.float64, device=dev)
        every = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(every, t)                      # every rank's own time: a slow rank is visible in the line
        share_ms = [float(x[0].item()) / steps * 1e3 for x in every]
        dt, dt_each = max(float(x[0].item()) for x in every), max(float(x[1].item()) for x in every)
    if rank != 0:
        return None
    pay, ack, itm = out
    # what the model of measured pieces says this N should cost (parallel.SLOT_MODEL) -- for the loopback run: the model of
    # the V real ranks it stands in for, NOT of the loopback itself (one GPU decodes every share there)
    shares_seg = [int(sum(segs[a:b])) for a, b in sh.tb_ranges]
    shares_llr = [int(co[b] - co[a]) * 2 for a, b in sh.tb_ranges]
    shares_res = [int(po[b] - po[a]) + 5 * int(b - a) for a, b in sh.tb_ranges]
    pred = parallel.predict_slot_ms(shares_seg, shares_llr, shares_res, chunks=sh.chunks)
    ok = bool(ack.all().item()) and all(torch.equal(pay[po[i]:po[i] + A // 8], payload[po[i]:po[i] + A // 8]) for i in range(n_tb))
    return {"loopback_virtual_ranks": loop, "rccl_p2p_bytes": int(sh.p2p_bytes), "rccl_p2p_bytes_per_slot": int(sh.p2p_bytes // (steps + 2)),
            "workload": "64 PUSCH transport blocks of one slot (273 PRB x 13 symbols, 64QAM, TBS 213 176 bit: 1664 code "
                        "segments) arriving on rank 0: scatter LLRs -> UL-SCH chain on every rank -> gather payloads/ACKs",
            "scaling": "strong", "n_gpus": world, "transport_blocks_per_rank": [int(b - a) for a, b in sh.tb_ranges],
            "pipeline_chunks_per_rank": [len(c) - 1 for c in sh.chunk_cut],
            "segments_per_rank": [int(sum(segs[a:b])) for a, b in sh.tb_ranges],
            "llr_bytes_per_rank": [int(co[b] - co[a]) * 2 for a, b in sh.tb_ranges],
            "ms_per_slot_per_rank": share_ms,
            "timing": "ms_per_slot: K slots enqueued back to back, one synchronize (max over ranks of the host clock); "
                      "ms_per_slot_events_rank0: a HIP event pair on the chain's stream around the same K slots; "
                      "ms_per_slot_synchronised_each: one slot, synchronize, next slot",
            "ms_per_slot_events_rank0": ev_ms / steps, "ms_per_slot_synchronised_each": dt_each / steps * 1e3,
            # (round 4's lines carried the synchronised figure under "ms_per_slot", round 5's the back-to-back one: both are
            # spelled out now, "ms_per_slot" stays what round 5 made it and says so -- ADVICE r05)
            "ms_per_slot_is": "back_to_back", "ms_per_slot_back_to_back": dt / steps * 1e3,
            "steps": steps, "ms_per_slot": dt / steps * 1e3, "info_gbps": n_tb * A * steps / dt / 1e9,
            "info_gbps_synchronised_each": n_tb * A * steps / dt_each / 1e9,
            "predicted_ms": pred["predicted_ms"], "predicted_ms_range": pred.get("predicted_ms_range"),
            "prediction": {"for_ranks": len(shares_seg), "bound": pred["bound"], "assumptions": pred.get("assumptions"),
                           "model": "openairinterface5g_amd/parallel.py predict_slot_ms: measured chain time by segments per call "
                                    "(profiles/r05/tb_latency.txt) + RCCL group overhead from the loopback slot + ASSUMED 50 GB/s "
                                    "per xGMI link and direction; N = 1: the chain call alone.  Weak scaling (the headline "
                                    "`value`): N x the N = 1 figure, no exchange on the data path",
                           "slowest_peer": pred.get("slowest_peer")},
            "coded_gbps": n_tb * G * steps / dt / 1e9, "llr_bytes_scattered": int(co[-1]) * 2,
            "all_ack_and_payload_equal": ok, "max_passes": int(itm.max().item())}


def chain_roofline(pkg, torch):
    """The memory-bound kernel of the path on the driver's own box: the UL-SCH chain's de-matching step (de-interleave +
    rate de-match with HARQ combining + int8 pack; nr_rate_matching.c:310-388, 507-603, nr_ulsch_decoding.c:195-210) for
    one slot of BASELINE configs[4] (64 transport blocks, 1664 segments), device-resident.  Algorithmic bytes from the job
    list: per segment E int16 LLRs in, n = max(Ncb, positions the decoder reads) int16 soft values out (and in, on a
    retransmission), ncols*Zc int8 decoder input out.  Time: HIP events around the kernel on its stream
    (nrLDPC_hip_chain_timing), the separate de-matching launch (NRLDPC_HIP_TB_FUSED=0) -- in the default path the same
    code is the prologue of the fused segment kernel, whose duration is reported beside it."""
    m = pkg.ldpc
    A = 213176
    while m.nr_segmentation(A + 24, 1) is None:
        A += 8
    G = (12 * 13 - 6) * 273 * 6
    n_tb = 64
    tbs = [dict(A=A, G=G, BG=1, Qm=6, Nl=1, rv=0, tbslbrm=0, round=0) for _ in range(n_tb)]
    po, co, ho, segs = m.tb_layout(tbs)
    g = torch.Generator(device="cuda").manual_seed(77)
    payload = torch.randint(0, 256, (int(po[-1]) + 16,), dtype=torch.uint8, device="cuda", generator=g)
    coded = torch.zeros(int(co[-1]) + 16, dtype=torch.uint8, device="cuda")
    m.PreparedTbBatch(tbs, payload, coded).encode()
    llr = ((1.0 - 2.0 * coded.float()) * 10 + 1.8 * torch.randn(coded.numel(), device="cuda", generator=g)).round().clamp(-127, 127).to(torch.int16)
    harq = torch.zeros(int(ho[-1]) + 16, dtype=torch.int16, device="cuda")
    pay_out = torch.zeros_like(payload)
    ack = torch.zeros(n_tb, dtype=torch.uint8, device="cuda")
    itm = torch.zeros(n_tb, dtype=torch.int32, device="cuda")
    dec = m.PreparedTbBatch(tbs, pay_out, llr, harq, ack, itm)
    dec.decode()
    torch.cuda.synchronize()
    # per-segment geometry, as the library derives it
    sg = m.nr_segmentation(A + 24, 1)
    Zc, C_ = sg["Z"], sg["C"]
    llr_len = 0
    alg = 0
    for r in range(C_):
        E = m.nr_get_E(G, C_, 6, 1, r)
        R, llr_len = m.nr_get_R_ldpc_decoder(0, E, 1, Zc, llr_len, 0)
        # columns the chain decodes the segment on: the rate mode's, cut behind the last one a first transmission reaches
        ncols = m.ulsch_decoder_columns(1, Zc, C_, sg["F"], sg["K"], 0, 0, E, 0, R)
        n = max(66 * Zc, ncols * Zc - 2 * Zc)
        alg += 2 * E + 2 * n + ncols * Zc
    alg *= n_tb
    res = {"kernel": "tb_rx_dematch_kernel", "bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s", "segments": int(sum(segs)),
           "algorithmic_bytes_per_launch": int(alg),
           "model": "per segment: E int16 in + max(Ncb, decoder positions) int16 soft values out + ncols*Zc int8 out (first "
                    "transmission: the soft buffer is cleared, not read; ncols = nrLDPC_hip_ulsch_decoder_columns: the rate "
                    "mode cut behind the last column that receives anything)"}
    prev = os.environ.get("NRLDPC_HIP_TB_FUSED")
    try:
        for mode, key in (("0", "dematch_us"), ("1", "fused_segment_kernel_us")):
            os.environ["NRLDPC_HIP_TB_FUSED"] = mode
            for _ in range(3):
                dec.decode()
            torch.cuda.synchronize()
            m.chain_timing(True)
            ts = []
            for _ in range(12):
                dec.decode()
                ts.append(m.chain_timing(True, read=True))
            m.chain_timing(False)
            ts = np.array(ts)
            if mode == "0":
                res["dematch_us"] = float(np.median(ts[:, 0]))
                res["decoder_us"] = float(np.median(ts[:, 1]))
                res["reassembly_verdict_us"] = float(np.median(ts[:, 2]))
            else:
                res["fused_segment_kernel_us"] = float(np.median(ts[:, 1]))
    finally:
        if prev is None:
            os.environ.pop("NRLDPC_HIP_TB_FUSED", None)
        else:
            os.environ["NRLDPC_HIP_TB_FUSED"] = prev
    res["achieved"] = alg / (res["dematch_us"] * 1e-6) / 1e9
    res["frac"] = res["achieved"] / HBM_PEAK_GBS
    res["all_ack"] = bool(ack.all().item())
    return res


def build_identity(pkg):
    """What ran: the library's version string, the sha256 of the shared object this process loaded and of the decoder
    kernel's sources it was built from -- compared with what profiles/hbm_traffic.json says the PMC passes measured."""
    import hashlib
    lib = Path(pkg.ldpc.LIB_PATH)
    src = hashlib.sha256()
    for n in ("ldpc_dec_fast_core.h", "ldpc_dec_fast_block.h", "ldpc_decoder_fast.hip", "ldpc_graph.c", "ldpc_graph.h"):
        src.update((ROOT / "openairinterface5g_amd" / "csrc" / n).read_bytes())
    return {"version": pkg.load_library().nrLDPC_hip_version().decode(), "lib_sha256": hashlib.sha256(lib.read_bytes()).hexdigest()[:16],
            "decoder_source_sha256": src.hexdigest()[:16]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-operating-point", action="store_true",
                    help="fixed-work launches only (used under rocprofv3 so that its per-kernel average covers one regime)")
    ap.add_argument("--kernel", type=int, default=0, help="0 = best kernel for the code, 1 = generic kernel")
    ap.add_argument("--no-strong", action="store_true", help="skip the strong-scaling slot measurement (configs[4])")
    ap.add_argument("--no-chain", action="store_true", help="skip the chain_roofline measurement (de-matching kernel, configs[4])")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last step (rank 0) as DIR/<name>.npy")
    args = ap.parse_args()

    import torch
    import openairinterface5g_amd as pkg

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher -- one rank per GPU under torch.distributed.run, the same
        # command line the driver uses (rendezvous on 127.0.0.1, a free port); the ranks' rank-0 JSON line is our output
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        os.execv(sys.executable, [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
                                  "--master-addr", "127.0.0.1", "--master-port", str(port), str(Path(__file__).resolve())]
                 + sys.argv[1:])
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with --nproc-per-node {args.gpus}")
    os.environ["NRLDPC_HIP_DEVICE"] = str(local_rank)   # (device-buffer calls run on the tensors' own GPU in any case)
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1 or os.environ.get("BENCH_FORCE_DIST") == "1":   # (the knob exercises the RCCL path on a 1-GPU box)
        import datetime
        import torch.distributed as dist
        if world == 1:                                   # BENCH_FORCE_DIST on one GPU: a rendezvous of one
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29533")
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        # a rank that dies inside a collective must not leave the others waiting for ever: the watchdog
        # turns a 3-minute stall into an error on every rank
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank), timeout=datetime.timedelta(seconds=180))
    pkg.LDPCinit()

    # ---- inputs resident in HBM ---------------------------------------------------------------------
    _, llr_fixed = make_batch(pkg, torch, -12.0, 1000 + rank)
    info_op, llr_op = make_batch(pkg, torch, 1.0, 2000 + rank)
    out = torch.zeros((BATCH, NUM_LLR // 8), dtype=torch.uint8, device="cuda")
    n_iter = torch.zeros(BATCH, dtype=torch.int32, device="cuda")

    def step(llr):
        pkg.decode_batch_device(BG, Z, R, llr, out, n_iter, numMaxIter=MAX_ITER, kernel=args.kernel)

    def timed(llr, steps, warmup):
        for _ in range(warmup):
            step(llr)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        # opening bracket: every rank has finished its warm-up and is idle
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        for i in range(steps):
            step(llr)
            ev[i + 1].record()
        # closing bracket: this rank's K steps are complete; the job time is the MAX over ranks (all_reduce below),
        # taken before the closing barrier so that the collective's own latency is not billed to the K steps
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        kern_ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]
        per_rank = [dt]
        if dist is not None:
            dist.barrier()
            t = torch.tensor([dt], dtype=torch.float64, device="cuda")
            every = [torch.zeros_like(t) for _ in range(world)]
            dist.all_gather(every, t)                       # the job time is the MAX; the others are kept for the line
            per_rank = [float(x.item()) for x in every]
            dt = max(per_rank)
        timed.per_rank_ms = [x / steps * 1e3 for x in per_rank]
        return dt, kern_ms

    def settle(llr):
        """Untimed launches until the GPU's clocks have come up.  After an idle period (process start, set-up on the host)
        the clocks ramp for ~30 ms of continuous work (profiles/r06/clock_ramp.txt: 0.417 -> 0.376 ms per launch); the
        driver's W = 5 warm-up steps are 2 ms.  Chunks of 25 launches, event-timed, until a chunk is no longer 0.5 % faster
        than the one before it (twice), at most 40 chunks.  Nothing of this is inside a timed region; the W warm-up steps
        and the K timed steps follow as the contract says.  BENCH_NO_SETTLE=1 switches it off."""
        chunks = []
        if os.environ.get("BENCH_NO_SETTLE") == "1":
            return chunks
        flat = 0
        while len(chunks) < 40 and flat < 2:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(25):
                step(llr)
            e1.record()
            e1.synchronize()
            chunks.append(e0.elapsed_time(e1) / 25)
            flat = flat + 1 if len(chunks) > 1 and chunks[-1] > 0.995 * chunks[-2] else 0
        return chunks

    if dist is not None:   # first collectives set up the communicator: keep that out of every timed region
        dist.barrier()
        torch.cuda.synchronize()

    # ---- the same K steps right after set-up, clocks still ramping (what rounds 1-5's lines measured) ---
    dt_cold, _ = timed(llr_fixed, args.steps, args.warmup)
    cold = {"ms_per_step": dt_cold / args.steps * 1e3, "gbps": world * args.steps * BATCH * N_TX / dt_cold / 1e9,
            "what": "W warm-up + K timed steps taken first, straight after set-up: the GPU's clocks are still ramping "
                    "(profiles/r06/clock_ramp.txt); rounds 1-5 reported this figure as `value`"}
    settle_ms = settle(llr_fixed)
    cold["settle_launches"] = 25 * len(settle_ms)
    cold["settle_ms_per_launch_first_last"] = [settle_ms[0], settle_ms[-1]] if settle_ms else None

    # ---- headline: fixed work (all 9 passes) ----------------------------------------------------------
    dt, kern_ms = timed(llr_fixed, args.steps, args.warmup)
    per_rank_ms_per_step = list(timed.per_rank_ms)
    if args.dump_outputs and rank == 0:
        # the headline's last step, as a caller of LDPCdecoder_batch receives it: the packed hard decisions of every block
        # and its pass count (inputs are seeded, so two builds can be compared output for output; 13.4 MB as float32)
        dump = Path(args.dump_outputs)
        dump.mkdir(parents=True, exist_ok=True)
        np.save(dump / "decoded_bits.npy", out.cpu().numpy().astype(np.float32))
        np.save(dump / "n_iter.npy", n_iter.cpu().numpy().astype(np.float32))
    passes_fixed = float(n_iter.float().mean().item())
    value = world * args.steps * BATCH * N_TX / dt / 1e9
    kern_avg_s = float(np.mean(kern_ms)) / 1e3

    # ---- operating point: Es/N0 = 1 dB, early stop on parity check ------------------------------------
    op = None
    if not args.no_operating_point:
        # a launch of this leg is 0.24 ms: with K // 2 steps (10 at the driver's K = 20) the closing synchronize() and the host
        # clock were 4 % of the figure; the leg takes its own step count (it is not the contract's timed region)
        op_steps = max(40, args.steps)
        dt_op, _ = timed(llr_op, op_steps, 2)
        it_h = n_iter.cpu().numpy()
        ok = it_h <= MAX_ITER
        good = ok & (out[:, :K // 8] == info_op).all(dim=1).cpu().numpy()
        stats = torch.tensor([float((~good).sum()), float(it_h.sum()), float(BATCH)], dtype=torch.float64, device="cuda")
        if dist is not None:
            dist.all_reduce(stats)                          # result gather, outside every timed region
        op = {"snr_db": 1.0, "gbps": world * op_steps * BATCH * N_TX / dt_op / 1e9, "steps": op_steps,
              "ms_per_step": dt_op / op_steps * 1e3,
              "bler": float(stats[0] / stats[2]), "mean_passes": float(stats[1] / stats[2])}

    def emit(strong, chain, devices, with_cpu):
        """rank 0: the ONE JSON line of the run"""
        traffic, pmc = None, {}
        tf = ROOT / "profiles" / "hbm_traffic.json"     # PMC-measured per-launch figures, if collected
        if tf.exists():
            try:
                pmc = json.loads(tf.read_text())
                traffic = pmc.get("ldpc_dec_bg1_z384_r13_b1024_bytes_per_launch")
            except Exception:
                traffic, pmc = None, {}
        # The decoder keeps every message in LDS: what it must move through HBM is the LLRs in and the bits out (A_min,
        # SURVEY 8d); that is the algorithmic byte count of the roofline entry, and the PMC traffic agrees with it.
        # The reference's dataflow (messages through memory, A_msg) is reported beside it, and so is the resource that
        # actually binds the kernel (VALU issue).
        achieved = BATCH * A_MIN / kern_avg_s / 1e9
        binding = {"name": "VALU issue (messages never leave LDS; HBM is idle 99 % of the time)"}
        ident = build_identity(pkg)
        # the PMC file is a tracked artefact of an earlier GPU run: say whether it was collected on the decoder this run
        # executed (same kernel sources) and on this very shared object
        measured = pmc.get("measured_on") or {}
        binding["counters_measured_on"] = measured or None
        binding["stale"] = measured.get("decoder_source_sha256") != ident["decoder_source_sha256"]
        binding["same_shared_object"] = measured.get("lib_sha256") == ident["lib_sha256"]
        if pmc.get("valu_wave_insts_per_launch"):
            n_simd = 256 * 4
            # mean issue time per VALU instruction: derived by tools/valu_issue_model.py (disassembly opcode histogram x
            # micro-benchmarked per-opcode rates), recorded with the counters by tools/make_traffic_json.py
            avg_ns = pmc.get("valu_avg_ns_per_wave_inst_per_simd") or 1.43
            t_issue = pmc["valu_wave_insts_per_launch"] / n_simd * avg_ns * 1e-9
            # of the issued VALU wave-instructions, the part that is check-node / bit-node arithmetic: 32 per (edge, 4-lane
            # item, pass) = the instruction count of the two bodies (profiles/r04/README.md (b)); the rest is item decoding,
            # task / record unpacking, masks, partly filled tasks, prologue, hard decision -- the target of any further work
            arith = EDGES * (Z // 4) * 32 // 64 * PASSES_FIXED * BATCH      # (wave-instructions: 64 items per wave)
            binding.update({"valu_wave_insts_per_launch": pmc["valu_wave_insts_per_launch"],
                            "issue_time_at_measured_opcode_rates_ms": t_issue * 1e3, "frac": t_issue / kern_avg_s,
                            "cn_bn_arithmetic_wave_insts_per_launch": arith,
                            "overhead_frac": 1.0 - arith / pmc["valu_wave_insts_per_launch"]})
        line = {
            "metric": "ldpc_decoder_coded_throughput", "value": value, "unit": "Gb/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
            "ms_per_step_per_rank": per_rank_ms_per_step,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "int8", "data": "synthetic",
            "config": {"workload": "BG1 Zc=384 R=1/3 numMaxIter=8 flooding min-sum, 1024 code blocks per GPU per step, "
                                   "fixed work (Es/N0=-12 dB: all 9 passes run), parity-check stop mode",
                       "blocks_per_gpu": BATCH, "coded_bits_per_block": N_TX, "mean_passes": passes_fixed,
                       "parallelism": f"blocks sharded over {world} GPU(s), no data-path collective"},
            "after_idle": cold,
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                         # `traffic` and binding_resource's counter figures are NOT measured in this run: rocprofv3 PMC
                         # passes cannot run inside it.  They come from the tracked file named here, collected on the
                         # build that binding_resource.counters_measured_on identifies (`stale` says if that is this one)
                         "traffic_source": "profiles/hbm_traffic.json (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, separate passes; "
                                           "tools/gpu_pmc.sh + tools/make_traffic_json.py)" if traffic is not None else None,
                         "model": "A_min: compulsory bytes = LLR in + bits out = 27 168 B/block (SURVEY 8d); the kernel is "
                                  "LDS-resident and NOT HBM bound -- see binding_resource",
                         "bytes_per_launch": BATCH * A_MIN, "kernel_avg_ms": kern_avg_s * 1e3,
                         "reference_dataflow": {"model": "A_msg: q read, r write, r read, q write per edge-lane and pass "
                                                         "+ LLR in + bits out = 4 395 552 B/block",
                                                "bytes_per_launch": BATCH * A_MSG,
                                                "GBs_at_this_speed": BATCH * A_MSG / kern_avg_s / 1e9,
                                                "frac_of_hbm_peak": BATCH * A_MSG / kern_avg_s / 1e9 / HBM_PEAK_GBS},
                         "binding_resource": binding},
            "chain_roofline": chain,
            "build": ident,
            "operating_point": op,
            "strong_scaling_slot": strong,
            # how the ranks were really run: the communicator's size (0 = no process group, plain single process) and
            # the HIP device ordinal of every rank
            "rccl_ranks": dist.get_world_size() if dist is not None else 0,
            "rank_devices": devices,
        }
        if with_cpu:                                    # rank 0 at N = 1 only
            line["cpu_baseline"] = cpu_baseline(llr_fixed[:256].cpu().numpy())
        print(json.dumps(line))

    # ---- strong scaling: one slot's transport blocks sharded over the ranks (configs[4]) --------------
    # The headline is measured by now.  Whatever the secondary legs do on a node nobody has run them on -- an exception
    # on one rank only, a point-to-point group that never completes -- must not cost that line: a deadline (shorter than
    # the process group's own watchdog, which aborts the process) prints the line with the leg marked as timed out and
    # ends every rank quietly.
    import threading

    def deadline_fire():
        try:
            if rank == 0:
                emit({"error": f"no result within {STRONG_DEADLINE_S} s: leg abandoned, headline line kept"}, None,
                     [local_rank], False)
                sys.stdout.flush()
        finally:
            os._exit(0)

    deadline = None
    if dist is not None:
        deadline = threading.Timer(STRONG_DEADLINE_S, deadline_fire)
        deadline.daemon = True
        deadline.start()
    strong = None
    if not args.no_strong:
        try:
            if os.environ.get("BENCH_TEST_STALL") == "1":   # (tests/test_bench.py: a leg that never comes back)
                time.sleep(10 * STRONG_DEADLINE_S)
            strong = strong_slot(pkg, torch, dist, world, rank, max(5, min(args.steps, 20)))
        except Exception as e:                      # the secondary experiment must not cost the headline line
            strong = {"error": f"{type(e).__name__}: {e}"[:300]}
            print(f"[bench] strong-scaling slot failed on rank {rank}: {strong['error']}", file=sys.stderr, flush=True)
    chain = None
    if not args.no_chain and rank == 0:
        try:
            chain = chain_roofline(pkg, torch)
        except Exception as e:
            chain = {"error": f"{type(e).__name__}: {e}"[:300]}
            print(f"[bench] chain_roofline failed: {chain['error']}", file=sys.stderr, flush=True)
    devices = [torch.cuda.current_device()]
    if dist is not None:
        ords = [None] * world
        dist.all_gather_object(ords, (rank, torch.cuda.current_device(), torch.cuda.get_device_properties(local_rank).name))
        devices = [o[1] for o in sorted(ords)]
    if deadline is not None:
        deadline.cancel()
    if rank == 0:
        emit(strong, chain, devices, not args.no_cpu_baseline and world == 1)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
