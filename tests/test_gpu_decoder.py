"""-m gpu: the HIP decoder through the C ABI vs the oracle (bit-exact: output bytes AND pass counts)."""
import numpy as np
import pytest

import oracle_lib as O
from common import (ALL_RATES, kbits, load_ref_code_words, load_ref_decoder_vectors, load_survey_decoder_vectors, make_llr,
                    random_info)

pytestmark = pytest.mark.gpu


def kernels_for(Z):
    """1 = generic kernel (any code); 3 / 4 = fast kernel (Zc % 4 == 0, Zc >= 8) in its throughput / latency workgroup
    shape (0 and 2 would pick the shape from the batch size); 5 = its multi-block variant; all must match the oracle."""
    if Z % 4 == 0 and 8 <= Z <= 64:
        return (1, 3, 4, 5)          # 5: several blocks per workgroup (small lifting sizes)
    if Z % 4 == 0 and Z >= 8:
        return (1, 3, 4)
    return (1, 5) if Z <= 30 else (1,)   # 5: four blocks interleaved byte-wise (any Zc)


def _compare(hip, BG, Z, R, llrs, it, mode=0, use_crc=False, E=0, ct=1):
    llr = np.stack(llrs)
    pre = np.full((llr.shape[0], (hip.ldpc.out_bytes(BG, Z, R, mode) + 3) // 4 * 4), 0x33, dtype=np.uint8)
    refs = [O.decode(BG, Z, R, llr[i], it, mode, use_crc, E, ct, out_init=0x33) for i in range(llr.shape[0])]
    for kern in kernels_for(Z):
        n_gpu, out_gpu = hip.decode_batch_host(BG, Z, R, llr, numMaxIter=it, outMode=mode, check_crc=use_crc, E=E,
                                               crc_type=ct, out=pre.copy(), kernel=kern)
        for i in range(llr.shape[0]):
            n_ref, out_ref = refs[i]
            assert n_ref == n_gpu[i], (kern, BG, Z, R, it, mode, use_crc, i, n_ref, int(n_gpu[i]))
            assert np.array_equal(out_ref, out_gpu[i]), (kern, BG, Z, R, it, mode, use_crc, i)


@pytest.mark.parametrize("BG", [1, 2])
def test_every_lifting_size_and_rate(hip, BG):
    """All 51 lifting sizes x 3 decoder-rate modes: noisy code words at two SNRs + random int8 LLRs."""
    rng = np.random.default_rng(100 + BG)
    for Z in O.LIFT_SIZES:
        for R in ALL_RATES[BG]:
            llrs = [make_llr(rng, BG, Z, R, -1.0), make_llr(rng, BG, Z, R, 1.0), make_llr(rng, BG, Z, R, "rand")]
            _compare(hip, BG, Z, R, llrs, 8)


@pytest.mark.parametrize("cfg", [(1, 384, 13), (1, 384, 23), (1, 384, 89), (1, 176, 13), (2, 64, 15), (2, 208, 13),
                                 (2, 208, 15), (2, 8, 15), (1, 2, 13), (2, 384, 23)])
def test_iteration_caps_modes_and_saturation(hip, cfg):
    BG, Z, R = cfg
    rng = np.random.default_rng(7 * Z + R)
    llrs = [make_llr(rng, BG, Z, R, k) for k in (-6.0, -1.5, -0.5, 0.5, 3.0, "rand", "sat")]
    llrs.append(np.zeros_like(llrs[0]))                      # all-zero input
    llrs.append(np.full_like(llrs[0], -128))                 # all -128
    llrs.append(np.full_like(llrs[0], 127))
    for it in (0, 1, 2, 3, 8, 20):
        _compare(hip, BG, Z, R, llrs, it)
    for mode in (1, 2):
        _compare(hip, BG, Z, R, llrs, 8, mode)


@pytest.mark.parametrize("cfg", [(1, 384, 13, 1), (1, 176, 23, 1), (2, 64, 15, 1), (2, 208, 13, 0), (2, 16, 23, 2),
                                 (1, 8, 89, 1)])
def test_crc_early_stop(hip, cfg):
    """check_crc != NULL: stop on CRC from pass 3 on (decoder.c:849-861), p_out untouched before."""
    BG, Z, R, ct = cfg
    rng = np.random.default_rng(11 * Z + R)
    K = kbits(BG, Z)
    crc_len = {0: 24, 1: 24, 2: 16}[ct]
    name = {0: "crc24a", 1: "crc24b", 2: "crc16"}[ct]
    llrs = []
    for snr in (-5.0, -1.0, 0.0, 1.0, 4.0):
        info = random_info(rng, BG, Z)
        crc = O.crc(name, info, K - crc_len) >> (32 - crc_len)
        for j in range(crc_len // 8):
            info[K // 8 - crc_len // 8 + j] = (crc >> (8 * (crc_len // 8 - 1 - j))) & 255
        llrs.append(make_llr(rng, BG, Z, R, snr, info))
    llrs.append(make_llr(rng, BG, Z, R, "rand"))
    llrs.append(np.zeros_like(llrs[0]))
    for it in (1, 2, 3, 8):
        _compare(hip, BG, Z, R, llrs, it, 0, True, K, ct)
    # E smaller than K (last bytes not covered)
    _compare(hip, BG, Z, R, llrs, 8, 0, True, K - 8 * 5, ct)


def test_survey_stage_vectors(hip):
    """Supplementary vectors recorded from the survey-stage reference build (see tools/dev_make_survey_vectors.py
    for their provenance: NOT the parity pin)."""
    for v in load_survey_decoder_vectors():
        for kern in kernels_for(v["Z"]):
            pre = np.full((1, (v["out"].size + 3) // 4 * 4), 0x55, dtype=np.uint8)
            n, out = hip.decode_batch_host(v["BG"], v["Z"], v["R"], v["llr"][None, :], numMaxIter=v["numMaxIter"],
                                           outMode=v["outMode"], check_crc=v["use_crc"], E=v["E"],
                                           crc_type=v["crc_type"], out=pre, kernel=kern)
            assert n[0] == v["n_iter"], (kern, v)
            assert np.array_equal(out[0], v["out"]), (kern, v["BG"], v["Z"], v["R"], v["numMaxIter"], v["outMode"])


def test_reference_hybrid_decoder_vectors(hip):
    """tests/golden/ref_decoder.npz: runs of oracle/_ref's decoder -- set-up (nrLDPC_init) and every data-movement step
    (nrLDPC_mPass.h) reference-COMPILED, node arithmetic restated on the reference's buffer layouts -- on 17 codes,
    converging and failing inputs, iteration caps 1 / 2 / 8, the three output modes, parity and CRC stop: pass counts and
    every output byte, on every kernel that serves the code."""
    n = 0
    for v in load_ref_decoder_vectors():
        for kern in kernels_for(v["Z"]):
            pre = np.full((1, (v["out"].size + 3) // 4 * 4), v["out_init"], dtype=np.uint8)
            n_it, out = hip.decode_batch_host(v["BG"], v["Z"], v["R"], v["llr"][None, :], numMaxIter=v["numMaxIter"],
                                              outMode=v["outMode"], check_crc=v["use_crc"], E=v["E"],
                                              crc_type=v["crc_type"], out=pre, kernel=kern)
            assert n_it[0] == v["n_iter"], (kern, v["BG"], v["Z"], v["R"], v["numMaxIter"], v["outMode"], v["use_crc"])
            assert np.array_equal(out[0], v["out"]), (kern, v["BG"], v["Z"], v["R"], v["numMaxIter"], v["outMode"])
        n += 1
    assert n >= 400
    # the by-name symbol (resident server) on the parity-stop runs
    for v in load_ref_decoder_vectors():
        if v["use_crc"] or v["outMode"] != 0:
            continue
        p = hip.make_dec_params(v["BG"], v["Z"], v["R"], v["numMaxIter"])
        n_it, out = hip.LDPCdecoder(p, v["llr"], p_out=np.full(v["out"].size, v["out_init"], np.uint8))
        assert n_it == v["n_iter"] and np.array_equal(out, v["out"]), (v["BG"], v["Z"], v["R"], v["numMaxIter"])


def test_reference_code_words_are_accepted_by_every_kernel(hip):
    """Every code word of the reference-COMPILED encoder (tests/golden/ref_encoder.npz), sent noiselessly (punctured
    columns 0, the rest +-16), satisfies the parity checks of every HIP decoder kernel in every decoder-rate mode within
    a few passes and gives its information bits back: the decoders' graphs (rows, columns, shifts mod Zc) are the
    reference encoder's."""
    for v in load_ref_code_words():
        BG, Z = v["BG"], v["Z"]
        K = kbits(BG, Z)
        bits = np.concatenate([np.unpackbits(v["info"])[:2 * Z], v["coded"]])
        for R in ALL_RATES[BG]:
            n = O.NCOLS[(BG, R)] * Z
            llr = (16 * (1 - 2 * bits[:n].astype(np.int16))).astype(np.int8)
            llr[:2 * Z] = 0
            for kern in kernels_for(Z):
                n_it, out = hip.decode_batch_host(BG, Z, R, llr[None, :], numMaxIter=8, kernel=kern)
                assert n_it[0] <= 4, (kern, BG, Z, R, int(n_it[0]))
                assert np.array_equal(np.unpackbits(out[0])[:K], bits[:K]), (kern, BG, Z, R)


def test_caller_supplied_crc_predicate_is_called_like_the_reference_calls_it(hip, tmp_path):
    """t_nrLDPC_dec_params.check_crc that is neither the library's nrLDPC_hip_check_crc nor the host executable's
    `check_crc`: called on the host with (p_out, E, crc_type) after every pass >= 3 until it holds
    (nrLDPC_decoder.c:849-861).  First from C, without an oracle (tests/abi_check_crc.c); then with the oracle's CRC as the
    caller's predicate: pass counts and outputs of the oracle's CRC-stop decode, also where the GPU's own CRC cannot
    serve (E % 8 != 0, byte-per-bit output)."""
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "abi_check_crc"
    subprocess.run(["gcc", "-O2", "-I", str(root / "include"), str(root / "tests" / "abi_check_crc.c"), "-o", str(exe), "-ldl"],
                   check=True)
    r = subprocess.run([str(exe), str(hip.ldpc.LIB_PATH)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "abi_check_crc: OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]

    rng = np.random.default_rng(404)
    for BG, Z, R in ((1, 384, 13), (2, 208, 13), (1, 30, 89), (2, 64, 15)):
        K = kbits(BG, Z)
        llrs = [make_llr(rng, BG, Z, R, snr, random_info(rng, BG, Z, with_crc24b=True)) for snr in (3.0, 0.5, -5.0)]
        for mode, E in ((0, K), (1, K), (0, K - 5), (2, K - 16)):
            seen = []

            def pred(ptr, n, t):
                seen.append((n, t))
                return O.check_crc(np.ctypeslib.as_array(ptr, shape=(n // 8 + 4,)), n, t)
            for llr in llrs:
                n_ref, out_ref = O.decode(BG, Z, R, llr, 8, mode, True, E, O.CRC24_B, out_init=0x77)
                pre = np.full((1, (out_ref.size + 3) // 4 * 4), 0x77, np.uint8)
                seen.clear()
                n_it, out = hip.decode_batch_host(BG, Z, R, llr[None, :], numMaxIter=8, outMode=mode, check_crc=pred, E=E,
                                                  crc_type=O.CRC24_B, out=pre)
                assert n_it[0] == n_ref and np.array_equal(out[0], out_ref), (BG, Z, R, mode, E, int(n_it[0]), n_ref)
                assert len(seen) == n_ref - 2 and all(c == (E, O.CRC24_B) for c in seen)
                # the by-name symbol; and the library's own predicate where the GPU's CRC cannot serve (falls to the host path)
                p = hip.make_dec_params(BG, Z, R, 8, mode, pred, E, O.CRC24_B)
                n1, out1 = hip.LDPCdecoder(p, llr, p_out=np.full(out_ref.size, 0x77, np.uint8))
                assert n1 == n_ref and np.array_equal(out1, out_ref)
                p = hip.make_dec_params(BG, Z, R, 8, mode, True, E, O.CRC24_B)
                n2, out2 = hip.LDPCdecoder(p, llr, p_out=np.full(out_ref.size, 0x77, np.uint8))
                assert n2 == n_ref and np.array_equal(out2, out_ref), (BG, Z, R, mode, E)


def test_reference_entry_point_and_abort(hip):
    """LDPCdecoder(), the symbol the reference's callers use, incl. the TB abort protocol (decoder.c:190-193,556-559)."""
    BG, Z, R = 1, 176, 13
    rng = np.random.default_rng(9)
    good, bad = make_llr(rng, BG, Z, R, 2.0), make_llr(rng, BG, Z, R, "rand")
    p = hip.make_dec_params(BG, Z, R, 8)
    ab = hip.ldpc.decode_abort_t()
    n, out = hip.LDPCdecoder(p, good, ab=ab)
    n_ref, out_ref = O.decode(BG, Z, R, good, 8)
    assert n == n_ref <= 8 and np.array_equal(out, out_ref) and not ab.failed
    n, _ = hip.LDPCdecoder(p, bad, ab=ab)
    assert n == 9 and ab.failed                       # failure raises the TB-wide flag
    n, _ = hip.LDPCdecoder(p, good, ab=ab)
    assert n == 10                                    # numMaxIter + 2: sibling segments bail out
    # unaligned host pointers are fine
    buf = np.zeros(good.size + 3, dtype=np.int8)
    buf[3:] = good
    n, out = hip.LDPCdecoder(p, buf[3:])
    assert n == n_ref and np.array_equal(out, out_ref)


def test_abort_raised_by_another_thread_during_a_call(hip):
    """decoder.c:556-559: the decoder looks at the transport block's abort flag at every iteration, so a sibling segment
    that fails on another worker stops a decode that is already running.  Here: a block that cannot converge with
    numMaxIter = 250 (3 ms on one CU); another thread raises `ab` 0.3 ms into the call; the call comes back early with
    numMaxIter + 2 and leaves p_out alone.  (Resident-server path; with NRLDPC_HIP_SERVER=0 the flag is only looked at
    on entry.)"""
    import threading
    import time
    BG, Z, R = 1, 384, 13
    rng = np.random.default_rng(77)
    bad = make_llr(rng, BG, Z, R, "rand")
    p = hip.make_dec_params(BG, Z, R, 250)
    out = np.full(hip.ldpc.out_bytes(BG, Z, R), 0x6b, np.uint8)
    t0 = time.perf_counter()
    n_full, _ = hip.LDPCdecoder(p, bad, p_out=out.copy())
    t_full = time.perf_counter() - t0
    assert n_full == 251                              # never converges: all 251 passes
    if hip.ldpc.server_stats()["calls"] == 0:
        pytest.skip("resident server not in use")
    for _ in range(3):
        ab = hip.ldpc.decode_abort_t()

        def raise_it():
            time.sleep(0.0003)
            ab.failed = True
        th = threading.Thread(target=raise_it)
        th.start()
        t0 = time.perf_counter()
        n, o = hip.LDPCdecoder(p, bad, p_out=out.copy(), ab=ab)
        dt = time.perf_counter() - t0
        th.join()
        if n == 252:
            break
    assert n == 252 and (o == 0x6b).all(), (n, dt, t_full)
    assert dt < 0.7 * t_full, (dt, t_full)


def test_per_segment_entry_point_every_code_and_mode(hip):
    """LDPCdecoder() -- served by the resident kernel through the caller's mailbox (csrc/ldpc_server.h) -- for every
    lifting size and decoder-rate mode of both base graphs, every output mode, parity-check and CRC stop, several
    iteration caps: output bytes and pass counts equal the oracle's, and the calls really went through the server."""
    rng = np.random.default_rng(2024)
    before = hip.ldpc.server_stats()
    n_calls = 0
    for BG in (1, 2):
        for Z in O.LIFT_SIZES:
            for R in ALL_RATES[BG]:
                for kind in (-1.0, 1.5, "rand"):
                    llr = make_llr(rng, BG, Z, R, kind)
                    p = hip.make_dec_params(BG, Z, R, 8)
                    n, out = hip.LDPCdecoder(p, llr, p_out=np.full(hip.ldpc.out_bytes(BG, Z, R), 0x33, np.uint8))
                    n_ref, out_ref = O.decode(BG, Z, R, llr, 8, out_init=0x33)
                    assert n == n_ref and np.array_equal(out, out_ref), (BG, Z, R, kind, n, n_ref)
                    n_calls += 1
    for (BG, Z, R, ct) in [(1, 384, 13, 1), (1, 176, 23, 1), (2, 64, 15, 1), (2, 208, 13, 0), (2, 16, 23, 2), (1, 8, 89, 1),
                           (1, 6, 13, 1)]:
        K = kbits(BG, Z)
        for it in (0, 1, 2, 3, 8, 20):
            for kind in (-2.0, 0.0, 2.0, "sat"):
                info = random_info(rng, BG, Z, with_crc24b=(ct == 1))
                llr = make_llr(rng, BG, Z, R, kind, info)
                for mode in (0, 1, 2):
                    p = hip.make_dec_params(BG, Z, R, it, outMode=mode)
                    n, out = hip.LDPCdecoder(p, llr, p_out=np.full(hip.ldpc.out_bytes(BG, Z, R, mode), 0x33, np.uint8))
                    n_ref, out_ref = O.decode(BG, Z, R, llr, it, mode, out_init=0x33)
                    assert n == n_ref and np.array_equal(out, out_ref), (BG, Z, R, it, kind, mode)
                    n_calls += 1
                if K % 8 == 0:
                    p = hip.make_dec_params(BG, Z, R, it, check_crc=True, E=K, crc_type=ct)
                    n, out = hip.LDPCdecoder(p, llr, p_out=np.full(hip.ldpc.out_bytes(BG, Z, R), 0x33, np.uint8))
                    n_ref, out_ref = O.decode(BG, Z, R, llr, it, 0, True, K, ct, out_init=0x33)
                    assert n == n_ref and np.array_equal(out, out_ref), (BG, Z, R, it, kind, "crc")
                    n_calls += 1
    after = hip.ldpc.server_stats()
    assert after["status"] == 0 and after["calls"] - before["calls"] == n_calls, (before, after, n_calls)


def test_per_segment_calls_with_an_all_zero_tail_run_on_the_cut_graph_and_say_the_same(hip):
    """What nr_ulsch_decoding.c hands LDPCdecoder() for a high-rate first transmission: the decoder input of the rate mode
    nr_get_R_ldpc_decoder chose, with the columns behind the last received value all zero.  In CRC-stop mode the library serves
    such a call on the mode cut behind its last non-zero column (ldpc_graph.h LDPC_R_COLS); the oracle runs the whole mode:
    pass counts and EVERY output byte of the whole mode's row (zeros behind the cut) must be equal -- converging and lost
    blocks, several iteration caps, tails that end inside a column, at a column edge, nowhere (no cut) and everywhere."""
    rng = np.random.default_rng(77)
    n_cut = 0
    for (BG, Z, R, ct) in [(1, 384, 23, 1), (1, 384, 13, 1), (1, 176, 23, 1), (2, 208, 13, 1), (2, 64, 15, 1), (1, 96, 89, 1), (2, 16, 23, 2)]:
        K, ncols, ncore = kbits(BG, Z), O.NCOLS[(BG, R)], 26 if BG == 1 else 14
        if K % 8:
            continue
        for keep_cols in (ncore - 1.5, ncore + 0.3, ncore + 1.0, ncore + 2.6, (ncore + ncols) / 2, ncols - 0.01, ncols):
            for kind in (1.0, 4.0, 9.0):
                info = random_info(rng, BG, Z, with_crc24b=(ct == 1))
                llr = make_llr(rng, BG, Z, R, kind, info)
                llr[int(keep_cols * Z):] = 0
                for it in (2, 3, 8):
                    p = hip.make_dec_params(BG, Z, R, it, check_crc=True, E=K, crc_type=ct)
                    n, out = hip.LDPCdecoder(p, llr, p_out=np.full(hip.ldpc.out_bytes(BG, Z, R), 0x33, np.uint8))
                    n_ref, out_ref = O.decode(BG, Z, R, llr, it, 0, True, K, ct, out_init=0x33)
                    assert n == n_ref and np.array_equal(out, out_ref), (BG, Z, R, keep_cols, kind, it, n, n_ref)
                n_cut += keep_cols < ncols - 1
    assert n_cut > 50


def test_bad_parameters(hip):
    with pytest.raises(RuntimeError):
        hip.decode_batch_host(1, 17, 13, np.zeros((1, 68 * 17), np.int8))       # 17 is not a lifting size
    with pytest.raises(KeyError):
        hip.decode_batch_host(1, 16, 15, np.zeros((1, 68 * 16), np.int8))       # rate 1/5 does not exist for BG1
    # zero blocks is a no-op
    n, out = hip.decode_batch_host(1, 16, 13, np.zeros((0, 68 * 16), np.int8))
    assert n.size == 0


def test_full_size_batch_properties_device(hip):
    """BASELINE config 2 at full size (1024 x BG1 Zc=384 R=1/3, 8-iteration cap) on device-resident buffers:
    encode -> AWGN -> decode round trip, syndrome of every decoded block, linearity (decoding is
    sign-symmetric: the all-zero code word with the same noise fails/succeeds identically), and a sample
    checked bit-exactly against the oracle."""
    import torch
    BG, Z, R, n = 1, 384, 13, 1024
    K = 22 * Z
    g = torch.Generator(device="cuda").manual_seed(1234)
    info = torch.randint(0, 256, (n, K // 8), dtype=torch.uint8, device="cuda", generator=g)
    coded = torch.empty((n, 66 * Z), dtype=torch.uint8, device="cuda")
    hip.encode_batch_device(BG, Z, info, coded)
    sigma = 1.0 / np.sqrt(2.0 * 10 ** (1.0 / 10.0))          # Es/N0 = 1 dB
    noise = torch.randn((n, 66 * Z), device="cuda", generator=g) * sigma
    def quant(y):
        return torch.clamp(torch.floor(y / (sigma / 16.0)), -128, 127).to(torch.int8)
    llr = torch.zeros((n, 68 * Z), dtype=torch.int8, device="cuda")
    llr[:, 2 * Z:] = quant(1.0 - 2.0 * coded.float() + noise)
    out = torch.zeros((n, 68 * Z // 8), dtype=torch.uint8, device="cuda")
    it = torch.zeros(n, dtype=torch.int32, device="cuda")
    out_g, it_g = torch.zeros_like(out), torch.zeros_like(it)
    hip.decode_batch_device(BG, Z, R, llr, out, it, numMaxIter=8)               # best kernel (fast)
    hip.decode_batch_device(BG, Z, R, llr, out_g, it_g, numMaxIter=8, kernel=1)  # generic kernel
    torch.cuda.synchronize()
    assert torch.equal(out, out_g) and torch.equal(it, it_g)                   # the two kernels agree on all 1024 blocks
    it_h, out_h, info_h = it.cpu().numpy(), out.cpu().numpy(), info.cpu().numpy()
    ok = it_h <= 8
    assert ok.mean() > 0.99, ok.mean()
    assert np.array_equal(out_h[ok][:, :K // 8], info_h[ok])                  # round trip
    # decoded words of converged blocks satisfy every parity check (core columns = systematic + core parity)
    for i in np.flatnonzero(ok)[:16]:
        bits = np.unpackbits(out_h[i])[:26 * Z]
        cw = O.encode(BG, Z, np.packbits(bits[:K]))
        assert np.array_equal(cw[K - 2 * Z:K - 2 * Z + 4 * Z], bits[K:K + 4 * Z])
    # bit-exact vs the oracle: a sample against the scalar restatement, ALL 1024 blocks against the vectorisable one
    # (itself checked against the scalar one for every code in tests/test_oracle.py)
    llr_h = llr.cpu().numpy()
    for i in list(range(0, n, 97)):
        n_ref, out_ref = O.decode(BG, Z, R, llr_h[i], 8)
        assert n_ref == it_h[i] and np.array_equal(out_ref, out_h[i]), i
    import os
    it_v, out_v = O.decode_mt(min(os.cpu_count() or 1, 32), BG, Z, R, llr_h, 8, vec=True)
    assert np.array_equal(it_v, it_h) and np.array_equal(out_v, out_h)
    # the host-buffer entry point splits a large batch into chunks on two streams (pageable and page-locked callers
    # take different copy paths): same results as the device-resident call, for batch sizes around the chunk edges
    pinned = torch.empty(llr.shape, dtype=torch.int8, pin_memory=True)
    pinned.copy_(llr)
    for src in (llr_h, pinned.numpy()):
        for nb in (1, 79, 80, 81, 161, 500):
            it_b, out_b = hip.decode_batch_host(BG, Z, R, src[:nb], numMaxIter=8)
            assert np.array_equal(it_b, it_h[:nb]) and np.array_equal(out_b, out_h[:nb]), nb
    # symmetry: same noise on the all-zero code word -> same pass counts, decoded word = 0
    llr0 = torch.zeros_like(llr)
    llr0[:, 2 * Z:] = quant(1.0 + noise * (1.0 - 2.0 * coded.float()))
    # (multiplying the noise by the BPSK sign maps the channel of word c onto the channel of word 0;
    #  floor() quantisation is not sign symmetric, so only statistics are compared)
    out0 = torch.zeros_like(out)
    it0 = torch.zeros_like(it)
    hip.decode_batch_device(BG, Z, R, llr0, out0, it0, numMaxIter=8)
    torch.cuda.synchronize()
    ok0 = (it0 <= 8).cpu().numpy()
    assert abs(ok0.mean() - ok.mean()) < 0.01
    assert int(out0[torch.from_numpy(ok0).cuda()][:, :K // 8].max()) == 0


@pytest.mark.parametrize("cfg", [(1, 384, 13, 257), (1, 384, 13, 701), (2, 384, 15, 513), (1, 352, 13, 300)])
def test_launches_of_several_workgroup_rounds_ragged_sizes_and_mixed_pass_counts(hip, cfg):
    """Launches of more than one workgroup round of the large codes (one workgroup per CU; double check-node tasks for the
    low-degree rows): block counts that do not fill the last round, noise levels from "converges in 3 passes" to "never" mixed in
    one launch (every workgroup finishes at another time), the launch repeated -- every block against the generic kernel, a
    sample against the oracle, and a one-pass cap."""
    import torch
    BG, Z, R, n = cfg
    K = (22 if BG == 1 else 10) * Z
    ncol = hip.ldpc.NCOLS[(BG, R)]
    g = torch.Generator(device="cuda").manual_seed(99 + n)
    info = torch.randint(0, 256, (n, K // 8), dtype=torch.uint8, device="cuda", generator=g)
    coded = torch.empty((n, (66 if BG == 1 else 50) * Z), dtype=torch.uint8, device="cuda")
    hip.encode_batch_device(BG, Z, info, coded)
    snr = torch.tensor([(-12.0, -1.0, 0.0, 0.5, 1.0, 2.0, 4.0)[i % 7] for i in range(n)], device="cuda")
    sigma = (1.0 / torch.sqrt(2.0 * 10 ** (snr / 10.0)))[:, None]
    y = 1.0 - 2.0 * coded.float() + sigma * torch.randn(coded.shape, device="cuda", generator=g)
    llr = torch.zeros((n, ncol * Z), dtype=torch.int8, device="cuda")
    llr[:, 2 * Z:] = torch.clamp(torch.floor(y / (sigma / 16.0)), -128, 127).to(torch.int8)
    out = torch.zeros((n, hip.ldpc.out_bytes(BG, Z, R)), dtype=torch.uint8, device="cuda")
    it = torch.zeros(n, dtype=torch.int32, device="cuda")
    out_g, it_g = torch.zeros_like(out), torch.zeros_like(it)
    hip.decode_batch_device(BG, Z, R, llr, out_g, it_g, numMaxIter=8, kernel=1)
    for rep in range(3):
        out.zero_()
        it.zero_()
        hip.decode_batch_device(BG, Z, R, llr, out, it, numMaxIter=8)
        torch.cuda.synchronize()
        assert torch.equal(it, it_g), rep
        assert torch.equal(out, out_g), rep
    it_h = it.cpu().numpy()
    assert len(set(it_h.tolist())) >= 3, np.bincount(it_h)       # the launch really mixes pass counts
    llr_h, out_h = llr.cpu().numpy(), out.cpu().numpy()
    for i in range(0, n, 41):
        n_ref, out_ref = O.decode(BG, Z, R, llr_h[i], 8, vec=True)
        assert n_ref == it_h[i] and np.array_equal(out_ref, out_h[i]), i
    # a one-pass cap
    hip.decode_batch_device(BG, Z, R, llr, out, it, numMaxIter=0)
    hip.decode_batch_device(BG, Z, R, llr, out_g, it_g, numMaxIter=0, kernel=1)
    torch.cuda.synchronize()
    assert torch.equal(it, it_g) and torch.equal(out, out_g)


@pytest.mark.parametrize("cfg", [(1, 384, 13), (1, 96, 23), (2, 208, 15), (2, 64, 13), (1, 32, 89), (2, 16, 23)])
def test_host_buffer_paths(hip, cfg):
    """LDPCdecoder_batch with mem = HOST: the decoder's workgroups pull their LLR rows over the link themselves -- from the
    caller's page-locked array in place (row pitches that are and are not multiples of 16 bytes) or from the library's
    staging area (pageable caller) -- and write bits / pass counts into the caller's arrays when those are page-locked,
    into staging rows otherwise; every combination equals the oracle, in parity-check and in CRC mode (where p_out of a
    block that stopped before pass 3 must stay untouched, decoder.c:849-861)."""
    import torch
    BG, Z, R = cfg
    rng = np.random.default_rng(1000 * BG + Z + R)
    n, K = 40, kbits(BG, Z)
    row = hip.ldpc.num_llr(BG, Z, R)
    ob = hip.ldpc.out_bytes(BG, Z, R, 0)
    infos = []
    for i in range(n):
        info = random_info(rng, BG, Z)
        crc = O.crc("crc24b", info, K - 24) >> 8
        info[K // 8 - 3:K // 8] = [(crc >> 16) & 255, (crc >> 8) & 255, crc & 255]
        infos.append(info)
    llrs = [make_llr(rng, BG, Z, R, float(rng.choice([-3.0, 0.5, 2.0, 6.0])), infos[i]) for i in range(n - 1)] + [np.zeros(row, np.int8)]
    for use_crc in (False, True):
        refs = [O.decode(BG, Z, R, llrs[i], 6, 0, use_crc, K if use_crc else 0, 1, out_init=0x5a) for i in range(n)]
        for pitch in (row, row + 4, (row + 15) // 16 * 16 + 16):
            for llr_pinned in (True, False):
                for out_pinned in (True, False):
                    src = torch.zeros((n, pitch), dtype=torch.int8, pin_memory=llr_pinned).numpy()
                    src[:, :row] = np.stack(llrs)
                    if pitch > row:
                        src[:, row:] = 99                       # never read
                    dst = torch.full((n, (ob + 3) // 4 * 4 + 8), 0x5a, dtype=torch.uint8, pin_memory=out_pinned).numpy()
                    it, out = hip.decode_batch_host(BG, Z, R, src, numMaxIter=6, check_crc=use_crc, E=K if use_crc else 0,
                                                    crc_type=1, out=dst)
                    for i in range(n):
                        assert refs[i][0] == it[i], (cfg, use_crc, pitch, llr_pinned, out_pinned, i, refs[i][0], int(it[i]))
                        assert np.array_equal(refs[i][1], out[i]), (cfg, use_crc, pitch, llr_pinned, out_pinned, i)
                    assert (dst[:, (ob + 3) // 4 * 4:] == 0x5a).all()


@pytest.mark.parametrize("cfg", [(1, 32, 13), (1, 8, 89), (2, 16, 15), (2, 48, 13), (1, 64, 23), (2, 24, 23),
                                 (1, 30, 13), (2, 15, 15), (1, 7, 89), (2, 2, 23), (1, 26, 23), (2, 4, 13), (1, 13, 13)])
def test_small_lifting_sizes_several_blocks_per_workgroup(hip, cfg):
    """Zc <= 64: a batch that fills the GPU is decoded with several code blocks per workgroup (ldpc_dec_fast_mblock.h):
    side by side for Zc % 4 == 0, four interleaved byte-wise for the other lifting sizes.  Blocks of one workgroup stop at
    different passes (mixed SNRs, some never), the last workgroup is partly filled, in parity-check and in CRC mode: all
    blocks equal the oracle, and the automatic choice (kernel 0) gives the same as the forced one (kernel 5)."""
    import torch
    BG, Z, R = cfg
    rng = np.random.default_rng(31 * Z + R + BG)
    K = kbits(BG, Z)
    per_wg = 64 // (Z // 4) if (Z % 4 == 0 and Z >= 8) else 4 * min(16, max(1, 64 // Z))
    n = 256 * (8 if Z <= 16 else 2) * min(per_wg, 64) + 37
    row = hip.ldpc.num_llr(BG, Z, R)
    base = []
    for i in range(24):
        inf = random_info(rng, BG, Z)
        if K >= 48:
            crc = O.crc("crc24b", inf, K - 24) >> 8
            inf[K // 8 - 3:K // 8] = [(crc >> 16) & 255, (crc >> 8) & 255, crc & 255]
        base.append(make_llr(rng, BG, Z, R, float(rng.choice([-4.0, -1.0, 0.5, 2.0, 5.0])), inf))
    base.append(make_llr(rng, BG, Z, R, "rand"))
    base.append(np.zeros(row, np.int8))
    idx = rng.integers(0, len(base), n)
    llr = torch.from_numpy(np.stack(base)[idx]).cuda()
    ob = hip.ldpc.out_bytes(BG, Z, R)
    modes = (False, True) if (K >= 48 and K % 8 == 0) else (False,)
    for use_crc in modes:
        refs = [O.decode(BG, Z, R, b, 8, 0, use_crc, K if use_crc else 0, 1, out_init=0x77) for b in base]
        exp_it = np.array([r[0] for r in refs], np.int32)[idx]
        exp_out = np.stack([r[1] for r in refs])[idx]
        for kern in (5, 0):
            out = torch.full((n, ob), 0x77, dtype=torch.uint8, device="cuda")
            it = torch.zeros(n, dtype=torch.int32, device="cuda")
            hip.decode_batch_device(BG, Z, R, llr, out, it, numMaxIter=8, check_crc=use_crc, E=K if use_crc else 0, crc_type=1, kernel=kern)
            torch.cuda.synchronize()
            it_h, out_h = it.cpu().numpy(), out.cpu().numpy()
            bad = np.nonzero(it_h != exp_it)[0]
            assert bad.size == 0, (cfg, use_crc, kern, int(bad[0]), int(exp_it[bad[0]]), int(it_h[bad[0]]), bad.size)
            bad = np.nonzero((out_h != exp_out).any(axis=1))[0]
            assert bad.size == 0, (cfg, use_crc, kern, int(bad[0]), bad.size)


def test_config3_mixed_bg2_batch_every_block(hip):
    """BASELINE configs[2] at full size: 256 blocks each of BG2 Zc=64 R=1/5, Zc=64 R=1/3, Zc=208 R=1/5, Zc=208 R=1/3
    (short URLLC-style blocks), in the waterfall so that pass counts spread from 2 to 9: every block's bits and pass
    count against the oracle, for both workgroup shapes of the fast kernel."""
    import os
    rng = np.random.default_rng(33)
    for (BG, Z, R) in ((2, 64, 15), (2, 64, 13), (2, 208, 15), (2, 208, 13)):
        n = 256
        llr = np.stack([make_llr(rng, BG, Z, R, float(rng.choice([-3.0, -1.0, 0.0, 2.0])), random_info(rng, BG, Z))
                        for _ in range(n)])
        it_ref, out_ref = O.decode_mt(min(os.cpu_count() or 1, 32), BG, Z, R, llr, 8, vec=True)
        assert len(set(it_ref.tolist())) >= 3, set(it_ref.tolist())
        for kern in (3, 4):
            it, out = hip.decode_batch_host(BG, Z, R, llr, numMaxIter=8, kernel=kern)
            assert np.array_equal(it, it_ref) and np.array_equal(out, out_ref), (BG, Z, R, kern)


def test_config3_as_one_mixed_call(hip):
    """BASELINE configs[2] as ONE call (LDPCdecoder_jobs): the 4 x 256 short BG2 blocks of the test above shuffled into
    one job array -- plus blocks of a lifting size the fast kernel does not take (Zc = 30: generic kernel) and one large
    BG1 block, so that the call spans workgroup shapes and both kernels -- every block with its own buffers; bits and
    pass counts of every block against the oracle, in parity-check and in CRC stop mode, submitted twice (the second
    submission reuses the job list)."""
    import os
    import torch
    m = hip.ldpc
    rng = np.random.default_rng(34)
    codes = [(2, 64, 15)] * 256 + [(2, 64, 13)] * 256 + [(2, 208, 15)] * 256 + [(2, 208, 13)] * 256 + [(2, 30, 15)] * 40 + [(1, 384, 13)] * 3
    order = rng.permutation(len(codes))
    for use_crc in (False, True):
        blocks, refs = [], []
        for k in order:
            BG, Z, R = codes[k]
            K = kbits(BG, Z)
            info = random_info(rng, BG, Z, with_crc24b=use_crc)
            llr = make_llr(rng, BG, Z, R, float(rng.choice([-3.0, -1.0, 0.0, 2.0])), info)
            E = K if use_crc else 0
            if use_crc and (K % 8 or K < 48):
                continue
            refs.append(O.decode(BG, Z, R, llr, 8, 0, use_crc, E, 1, vec=True))
            blocks.append(dict(BG=BG, Z=Z, R=R, E=E, crc_type=1, llr=torch.from_numpy(llr).cuda(),
                               out=torch.full((m.out_bytes(BG, Z, R),), 0x33, dtype=torch.uint8, device="cuda")))
        n_iter = torch.zeros(len(blocks), dtype=torch.int32, device="cuda")
        jobs = m.PreparedDecJobs(blocks, n_iter, check_crc=use_crc)
        for rep in range(2):
            n_iter.zero_()
            jobs.decode()
            torch.cuda.synchronize()
            it = n_iter.cpu().numpy()
            for i, (b, (n_ref, out_ref)) in enumerate(zip(blocks, refs)):
                assert it[i] == n_ref, (use_crc, rep, i, b["BG"], b["Z"], b["R"], int(it[i]), n_ref)
                if not use_crc or n_ref >= 3:
                    assert np.array_equal(b["out"].cpu().numpy(), out_ref), (use_crc, rep, i, b["BG"], b["Z"], b["R"])
        assert len(set(n_iter.cpu().numpy().tolist())) >= 3


def test_ldpctest_acceptance_and_seed_identical_bler(hip):
    """The reference CI's acceptance criterion for the library (`ldpctest -l{3872..8448} -s10 -n100` must print
    `BLER 0.000000`, cmake_targets/autotests/test_case_list.xml:68-94) on a subset, and -- on identical AWGN seeds --
    the very same per-block pass counts and BLER as the CPU oracle at a low SNR where blocks do fail."""
    import io
    import ldpctest_hip as T
    for length in (3872, 5632, 8448):
        buf = io.StringIO()
        res = T.run(T.parser().parse_args(["-l", str(length), "-s", "10", "-n", "25"]), out=buf)
        assert "BLER 0.000000" in buf.getvalue() and res[-1]["errors"] == 0
    args = ["-l", "8448", "-s", "0.0", "-t", "5", "-n", "12", "-i", "8", "-S", "2", "--seed", "77"]
    gpu = T.run(T.parser().parse_args(args), out=io.StringIO())
    cpu = T.run(T.parser().parse_args(args + ["--oracle"]), out=io.StringIO())
    assert gpu == cpu and gpu[0]["errors"] > 0


def test_ldpctest_beyond_the_ci_lengths(hip):
    """What ldpctest does outside the CI list (TESTBENCH/ldpctest.c:177-305): block lengths that are not Kb*Zc (the
    encoder is handed K = block_length, pads with zeros and cuts the code word to the mother rate), the punctured rates
    -r 2 -d 3 and -r 22 -d 25 (decoder modes R23 / R89), several segments per trial, and the one-trial encoder
    cross-check.  On identical seeds the library and the CPU oracle produce the same result records -- pass counts,
    block and bit errors -- whatever the reference's own bookkeeping makes of those lengths."""
    import io
    import ldpctest_hip as T
    for extra in (["-l", "6000"], ["-l", "3000"], ["-l", "500", "-S", "3"], ["-l", "8448", "-r", "2", "-d", "3", "-s", "4"],
                  ["-l", "8448", "-r", "22", "-d", "25", "-s", "7"], ["-l", "3872", "-r", "2", "-d", "3", "-s", "5", "-S", "9"],
                  ["-l", "1000", "-r", "1", "-d", "5", "-s", "1"]):
        args = extra + (["-s", "2"] if "-s" not in extra else []) + ["-t", "4", "-n", "6", "-i", "8", "--seed", "11"]
        gpu = T.run(T.parser().parse_args(args), out=io.StringIO())
        cpu = T.run(T.parser().parse_args(args + ["--oracle"]), out=io.StringIO())
        assert gpu == cpu and len(gpu) >= 1, (extra, gpu, cpu)
    buf = io.StringIO()                                      # -n 1: encoder cross-check, nothing may differ
    T.run(T.parser().parse_args(["-l", "6000", "-s", "10", "-n", "1", "-S", "9"]), out=buf)
    assert "differ in seg" not in buf.getvalue() and "BLER" in buf.getvalue()


def test_concurrent_callers_of_the_reference_entry_point(hip, tmp_path):
    """16 pthreads calling LDPCdecoder() at once with different codes / caps / stop modes (the reference's thread-pool
    usage): every concurrent call must return what it returned single-threaded -- through the resident server kernel
    (default; 16 callers on 64 slots, then 16 callers sharing 4 slots) and with one launch per call
    (NRLDPC_HIP_SERVER=0)."""
    import json
    import os
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "abi_threads"
    subprocess.run(["gcc", "-O2", "-I", str(root / "include"), str(root / "tests" / "abi_threads.c"), "-o", str(exe),
                    "-ldl", "-lpthread"], check=True)
    import abi_dump
    for extra in ({}, {"NRLDPC_HIP_SRV_SLOTS": "4", "NRLDPC_HIP_SRV_IDLE_US": "150"}, {"NRLDPC_HIP_SERVER": "0"}):
        dump = tmp_path / "abi_threads.dump"
        env = dict(os.environ, ABI_DUMP=str(dump), **extra)
        r = subprocess.run([str(exe), str(hip.ldpc.LIB_PATH), "16", "150"], capture_output=True, text=True, env=env,
                           timeout=300)
        assert r.returncode == 0, (extra, r.stderr[-2000:])
        d = json.loads(r.stdout.strip().splitlines()[-1])
        assert d["failures"] == 0 and d["calls"] == 2400, extra
        assert d["served"] == (0 if extra.get("NRLDPC_HIP_SERVER") == "0" else 2400 + 12), (extra, d)
        # ... and what they all returned is what the oracle returns for the same inputs (the C caller's view of the entry point)
        assert abi_dump.check_against_oracle(dump, 12) == d["iters"], extra


def test_server_generations_wait_modes_and_a_server_that_cannot_be_relaunched(hip, tmp_path):
    """The resident server's life cycle under the callers' feet.  (1) NRLDPC_HIP_SRV_IDLE_US=1: the generation is told to
    leave while calls are in flight (a 9-pass decode lasts ~120 us) and almost every call relaunches it -- requests rung
    into a dying generation are served by it or found by the next one; (2) the three ways a caller may wait
    (NRLDPC_HIP_SRV_WAIT); (3) fault injection: once the callers' threads start, the server cannot be launched any more -- the calls that were
    waiting come back NOT DECODED (numMaxIter + 1, p_out untouched: never a stale copy under a success code, VERDICT r02
    weak #4), every later call goes through the launch-per-call path, and all other results stay exact."""
    import json
    import os
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "abi_threads"
    subprocess.run(["gcc", "-O2", "-I", str(root / "include"), str(root / "tests" / "abi_threads.c"), "-o", str(exe),
                    "-ldl", "-lpthread"], check=True)

    def run(threads, calls, **extra):
        r = subprocess.run([str(exe), str(hip.ldpc.LIB_PATH), str(threads), str(calls)], capture_output=True, text=True,
                           env=dict(os.environ, **extra), timeout=600)
        assert r.returncode == 0, (extra, r.stdout[-500:], r.stderr[-2000:])
        return json.loads(r.stdout.strip().splitlines()[-1])

    d = run(8, 150, NRLDPC_HIP_SRV_IDLE_US="1")
    assert d["failures"] == 0 and d["nacked"] == 0 and d["served"] == 1200 + 12 and d["server_launches"] > 3, d
    for mode in ("spin", "yield", "sleep"):
        d = run(16, 100, NRLDPC_HIP_SRV_WAIT=mode)
        assert d["failures"] == 0 and d["served"] == 1600 + 12, (mode, d)
    d = run(8, 200, NRLDPC_HIP_SRV_IDLE_US="1", ABI_FAIL_LAUNCHES_FROM_NOW="1", ABI_ALLOW_NACK="1")
    assert d["failures"] == 0 and d["nacked"] >= 1 and d["served"] < 1600 + 12, d


def test_general_kernels_for_the_lifting_size_that_has_instantiations_of_its_own():
    """Zc = 384 (and 352, 320, 288, 256, 208: ldpc_kernels.h LDPC_FAST_ZC_LIST) runs on instantiations with compile-time row
    strides (ldpc_dec_fast_block.h ZC: batch, job-array and fused segment kernels); NRLDPC_HIP_ZC=0 sends it through the general
    kernels every other lifting size uses.  The tests that decode those sizes -- every lifting size and rate, code-block batches,
    mixed job arrays, both transport-block chains, the fused segment kernel against the four-launch path -- are run again that
    way: same oracle, same fixtures."""
    import os
    import subprocess
    import sys
    if os.environ.get("NRLDPC_HIP_ZC") == "0":
        pytest.skip("already the general-kernel run")
    env = dict(os.environ, NRLDPC_HIP_ZC="0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_decoder.py"),
                        os.path.join(root, "tests", "test_gpu_tb_chain.py"), os.path.join(root, "tests", "test_gpu_tb_resident.py"),
                        "-m", "gpu", "-q", "-x", "-k",
                        "every_lifting_size or iteration_caps or crc_early_stop or reference_hybrid or several_workgroup_rounds or ulsch_decode_matches "
                        "or harq_rounds or fused_segment_kernel_against or first_transmissions_on_the_cut_graph"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
