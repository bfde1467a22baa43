"""-m gpu: the plugin life cycle -- LDPCshutdown(), the relaunch of the resident server kernels behind LDPCdecoder /
LDPCencoder, process exit with a generation still on the GPU, and both plugin slots loaded the way the reference loads them
(RTLD_LAZY | RTLD_NODELETE | RTLD_GLOBAL, load_module_shlib.c:160; libldpc_hip_t2.so with and without the main library
loaded first).

LDPCshutdown is not the reference's no-op (csrc/ldpc_api.cpp): it asks both resident kernels to leave and waits for them,
keeps every device object, and promises that a later call starts the kernels again and that other threads may be inside a
call meanwhile.  The stop request is the host_stop branch of the server's poll loop (csrc/ldpc_server.hip).

Every GPU-using step is a fresh child process.  NRLDPC_HIP_SRV_IDLE_US is set to IDLE_US (seconds) in all of them: no
generation then leaves on its own, so launch counts are exact, and a stop request that the kernel does not see costs the whole
time-out where one that works costs microseconds to milliseconds.  The bounds on time below are IDLE / 4: they tell those two
apart on a loaded machine, they assert no latency.  The measured values are in DESIGN section 6."""
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import pytest

import abi_dump

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
IDLE_US = 4_000_000
IDLE_S = IDLE_US / 1e6
THREADS, CALLS = 8, 150


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("abi_lifecycle") / "abi_lifecycle"
    subprocess.run(["gcc", "-O2", "-I", str(ROOT / "include"), str(ROOT / "tests" / "abi_lifecycle.c"), "-o", str(exe),
                    "-ldl", "-lpthread"], check=True)
    return exe


def run_harness(exe, lib, tmp_path, **extra):
    """(report of the harness, seconds between its last stamp and its end)"""
    dump = tmp_path / "abi_lifecycle.dump"
    env = dict(os.environ, NRLDPC_HIP_SRV_IDLE_US=str(IDLE_US), **extra)
    r = subprocess.run([str(exe), str(lib), str(dump), str(THREADS), str(CALLS)], capture_output=True, text=True, env=env,
                       timeout=120)
    gone = time.time()
    assert r.returncode == 0, (extra, r.returncode, r.stdout[-1500:], r.stderr[-2000:])
    d = json.loads(r.stdout.strip().splitlines()[-1])
    print(extra, json.dumps(d), "gone %.3f s after the stamp" % (gone - d["exit_stamp"]))
    # what every comparison inside the harness was made with is the oracle's answer: 12 decoder calls (the CRC stop among
    # them), 1 + 3 + 8 encoder segments of BG1 Zc=384 and of BG2 Zc=208
    assert abi_dump.check_against_oracle(dump, 12, 24) == d["iters"], extra
    return d, gone - d["exit_stamp"]


@pytest.mark.parametrize("extra", [{}, {"NRLDPC_HIP_SRV_SLOTS": "4"}], ids=["64_slots", "4_shared_slots"])
def test_shutdown_relaunch_and_exit_from_a_c_caller(hip, harness, tmp_path, extra):
    """tests/abi_lifecycle.c: (a) shutdown before any call, twice, and a second LDPCinit; (b) the baseline, held against the
    oracle; (c) with a generation resident, LDPCshutdown returns at once, the next call is served by generation g0 + 1 with
    the same bytes, two shutdowns in a row cost one generation, the encoder's server likewise; (d) 8 threads x 150 calls
    with a shutdown every 100 completed calls: every call served by the server with the oracle's answer; (e) return from
    main with both kernels resident: the atexit handler gets them off the GPU."""
    d, exit_s = run_harness(harness, hip.ldpc.LIB_PATH, tmp_path, **extra)
    assert d["pre"] == [0, 0, 0, 0] and d["shutdown_rc"] == 0 and d["status"] == 0, d
    assert d["mismatches"] == 0 and d["enc_mismatches"] == 0, d
    # (c) the generation that served the baseline is still there, one shutdown = one relaunch, a double shutdown too
    assert d["g0"] >= 1 and d["g_control"] == d["g0"], d
    assert d["g_after_shutdown"] == d["g0"] + 1 and d["g_after_two_shutdowns"] == d["g0"] + 2, d
    assert max(d["shutdown_us"]) < IDLE_US / 4, d
    # (d)
    assert d["calls"] == THREADS * CALLS and d["shutdowns"] == THREADS * CALLS // 100 == 12, d
    assert d["failures"] == 0 and d["nacked"] == 0, d
    assert d["served"] == d["calls"], d                  # nothing fell back to the launch path
    assert d["server_launches"] >= 2, d
    assert d["shutdown_under_load_max_us"] < IDLE_US / 4, d
    # (e) the last generation is the one the exit handler has to stop
    assert d["g_exit"] >= d["g_after_two_shutdowns"] + d["server_launches"], d
    assert exit_s < IDLE_S / 4, (exit_s, d)


def test_shutdown_with_the_server_switched_off(hip, harness, tmp_path):
    """NRLDPC_HIP_SERVER=0 (one launch per call): LDPCshutdown is a no-op that returns 0, the same harness sees the same
    oracle-checked results, no call is served by a resident kernel and none is ever launched."""
    d, exit_s = run_harness(harness, hip.ldpc.LIB_PATH, tmp_path, NRLDPC_HIP_SERVER="0")
    assert d["pre"] == [0, 0, 0, 0] and d["shutdown_rc"] == 0, d
    assert d["mismatches"] == 0 and d["enc_mismatches"] == 0 and d["failures"] == 0 and d["nacked"] == 0, d
    assert d["served"] == 0 and d["server_launches"] == 0 and d["g_exit"] == 0 and d["shutdowns"] == 12, d
    assert max(d["shutdown_us"]) < IDLE_US / 4 and exit_s < IDLE_S / 4, (exit_s, d)


@pytest.mark.parametrize("mode", ["offload", "offload_alone", "chain", "inflight"])
def test_device_state_survives_shutdown(hip, mode):
    """tests/lifecycle_script.py: what the shutdown keeps.  offload: both libraries loaded as the reference loads them, four
    HARQ rounds of the offload slot with LDPCshutdown of both between the rounds -- the device soft buffer combines across them;
    offload_alone: libldpc_hip_t2.so opened by itself (the main library through DT_NEEDED + $ORIGIN), its four names taken from
    that handle compute the offload slot's semantics, not the main library's; chain: nrLDPC_hip_ulsch_decode with the library's
    soft buffers, a shutdown between round 0 (lost) and round 1, dlsch_encode plans before and after; inflight: a device-mode
    batch enqueued on a caller's stream, shutdown before it is synchronised."""
    env = dict(os.environ, NRLDPC_HIP_SRV_IDLE_US=str(IDLE_US))
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "lifecycle_script.py"), mode], capture_output=True, text=True, env=env,
                       cwd=str(ROOT), timeout=180)
    print(r.stdout[-500:])
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("ok " + mode), (mode, r.returncode, r.stdout[-1500:], r.stderr[-3000:])
