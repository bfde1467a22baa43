"""-m gpu: codeword scrambling and unscrambling on the GPU (nrLDPC_hip_codeword_scrambling / _unscrambling) against numpy
and the bit-serial Gold sequence of 38.211 5.2.1 (test_scrambling_host.serial_gold), in host and device memory; and the
transmit / receive chain around them: encode -> scramble -> channel -> unscramble -> decode."""
import numpy as np
import pytest

from test_gpu_tb_chain import make_tbs
from test_scrambling_host import c_init_of, serial_gold, words_of

import oracle_lib as O

pytestmark = pytest.mark.gpu


def scrambled_words(bits, n_rnti, q, n_id):
    """what nr_codeword_scrambling writes, with the bits behind the end zero"""
    n = bits.size
    c = serial_gold(c_init_of(n_rnti, q, n_id), n)
    pad = np.zeros(-n % 32, np.uint8)
    return words_of(np.concatenate([(bits & 1) ^ c, pad]))


def unscrambled(llr, n_rnti, q, n_id):
    c = serial_gold(c_init_of(n_rnti, q, n_id), llr.size)
    neg = (-llr.astype(np.int32)).astype(np.int16)  # -(-32768) wraps to -32768, as the reference's mullo by -1 does
    return np.where(c == 1, neg, llr).astype(np.int16)


SIZES = [1, 31, 32, 33, 1000, 32 * 1024 - 5, 32 * 1024, 32 * 1024 + 1, 245700, 1 << 21]
PARAMS = [(0, 0, 0), (0xFFFF, 1, 1023), (0x4601, 0, 17), (1, 1, 500)]


def test_scrambling_host_memory(hip):
    rng = np.random.default_rng(1)
    for i, n in enumerate(SIZES):
        p = PARAMS[i % len(PARAMS)]
        bits = rng.integers(0, 256, n, dtype=np.uint8)   # only bit 0 of a byte counts (the reference shifts it to the sign)
        got = hip.ldpc.codeword_scrambling(bits, p[1], p[2], p[0])
        assert np.array_equal(got, scrambled_words(bits, *p)), (n, p)


def test_scrambling_device_memory(hip):
    import torch
    rng = np.random.default_rng(2)
    for i, n in enumerate(SIZES):
        p = PARAMS[(i + 1) % len(PARAMS)]
        for off in (0, 3):                                 # an input that is not 16-byte aligned takes the byte loads
            bits = rng.integers(0, 2, n, dtype=np.uint8)
            src = torch.zeros(n + off, dtype=torch.uint8, device="cuda")
            src[off:] = torch.from_numpy(bits).cuda()
            nw = (n + 31) // 32
            out = torch.full((nw + 8,), -0x5a5a5a5b, dtype=torch.int32, device="cuda")   # sentinel behind the words
            hip.ldpc.codeword_scrambling(src[off:], p[1], p[2], p[0], out=out)
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(np.uint32)
            assert np.array_equal(got[:nw], scrambled_words(bits, *p)), (n, off, p)
            assert (got[nw:] == 0xA5A5A5A5).all()


def special_llrs(rng, n):
    llr = rng.integers(-32768, 32768, n).astype(np.int16)
    k = min(n, 64)
    llr[:k] = np.resize(np.array([32767, -32767, -32768, 0], np.int16), k)  # where c = 1 and where c = 0 among them
    return llr


def test_unscrambling_host_memory(hip):
    rng = np.random.default_rng(3)
    for i, n in enumerate(SIZES):
        p = PARAMS[i % len(PARAMS)]
        llr = special_llrs(rng, n + 40)
        ref = llr.copy()
        ref[:n] = unscrambled(llr[:n], *p)
        hip.ldpc.codeword_unscrambling(llr, p[1], p[2], p[0], size=n)
        assert np.array_equal(llr, ref), (n, p)                 # [n, n + 40) untouched


def test_unscrambling_device_memory(hip):
    import torch
    rng = np.random.default_rng(4)
    for i, n in enumerate(SIZES):
        p = PARAMS[(i + 2) % len(PARAMS)]
        for off in (0, 1):
            llr = special_llrs(rng, n + off + 40)
            t = torch.from_numpy(llr).cuda()
            hip.ldpc.codeword_unscrambling(t[off:], p[1], p[2], p[0], size=n)
            torch.cuda.synchronize()
            ref = llr.copy()
            ref[off:off + n] = unscrambled(llr[off:off + n], *p)
            assert np.array_equal(t.cpu().numpy(), ref), (n, off, p)


def test_invalid_parameters_write_nothing_on_the_device(hip):
    import torch
    L = hip.ldpc._scr_lib()
    bits = torch.ones(100, dtype=torch.uint8, device="cuda")
    out = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    llr = torch.arange(100, dtype=torch.int16, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for n_rnti, q, n_id in ((0x10000, 0, 0), (0, 2, 0), (0, 0, 1024)):
        assert L.nrLDPC_hip_codeword_scrambling(bits.data_ptr(), 100, q, n_id, n_rnti, out.data_ptr(), 1, s) < 0
        assert L.nrLDPC_hip_codeword_unscrambling(llr.data_ptr(), 100, q, n_id, n_rnti, 1, s) < 0
    torch.cuda.synchronize()
    assert (out.cpu() == 7).all() and torch.equal(llr.cpu(), torch.arange(100, dtype=torch.int16))


def test_transport_blocks_scrambled_and_back(hip):
    """The encoder chain's output scrambled per transport block, a channel on the scrambled bits (bit 0 -> +, bit 1 -> -,
    noise), the LLRs unscrambled, the decoder chain: every block decodes, and the transmitted words are the spec's."""
    rng = np.random.default_rng(5)
    tbs = [t for t in make_tbs() if t["rv"] in (0, 3)]
    pays = [rng.integers(0, 256, t["A"] // 8, dtype=np.uint8) for t in tbs]
    coded = hip.ldpc.dlsch_encode_host(tbs, pays)
    llrs = []
    for i, f in enumerate(coded):
        n_rnti, q, n_id = int(rng.integers(0, 0x10000)), i & 1, int(rng.integers(0, 1024))
        words = hip.ldpc.codeword_scrambling(f, q, n_id, n_rnti)
        assert np.array_equal(words, scrambled_words(f, n_rnti, q, n_id)), i
        tx = ((words[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.uint8).ravel()[:f.size]
        llr = ((1 - 2 * tx.astype(np.int16)) * 24 + rng.integers(-10, 11, f.size)).astype(np.int16)
        hip.ldpc.codeword_unscrambling(llr, q, n_id, n_rnti)
        llrs.append(llr)
    segs = [O.segmentation(None, O.len_with_crc(1, t["A"]), t["BG"])["C"] for t in tbs]
    harq = np.zeros((sum(segs), hip.ldpc.HARQ_STRIDE), np.int16)
    for t in tbs:
        t["round"] = 0
    out, ack, itm = hip.ldpc.ulsch_decode_host(tbs, llrs, harq)
    for i, t in enumerate(tbs):
        assert ack[i] and np.array_equal(out[i], pays[i]), (t, int(itm[i]))


def test_slot_of_64_transport_blocks_on_device_buffers(hip):
    """the 64-TB slot's shape (G = 245 700 per block): one call per block on device memory, back to back on one stream"""
    import torch
    rng = np.random.default_rng(6)
    G = 245700
    bits = rng.integers(0, 2, (64, G), dtype=np.uint8)
    src = torch.from_numpy(bits).cuda()
    nw = (G + 31) // 32
    out = torch.zeros((64, nw), dtype=torch.int32, device="cuda")
    llr = torch.from_numpy(special_llrs(rng, 64 * G).reshape(64, G)).cuda()
    llr_h = llr.cpu().numpy()
    for i in range(64):
        hip.ldpc.codeword_scrambling(src[i], i & 1, 1023 - i, 0x1000 + i, out=out[i])
        hip.ldpc.codeword_unscrambling(llr[i], i & 1, 1023 - i, 0x1000 + i)
    torch.cuda.synchronize()
    got, got_llr = out.cpu().numpy().view(np.uint32), llr.cpu().numpy()
    for i in (0, 1, 37, 63):
        p = (0x1000 + i, i & 1, 1023 - i)
        assert np.array_equal(got[i], scrambled_words(bits[i], *p)), i
        assert np.array_equal(got_llr[i], unscrambled(llr_h[i], *p)), i


def test_device_mode_needs_every_buffer_on_the_gpu(hip):
    """DEVICE mem: an `out` (or `in`) that is host memory is refused before anything is enqueued"""
    import torch
    L = hip.ldpc._scr_lib()
    s = torch.cuda.current_stream().cuda_stream
    bits_d = torch.ones(100, dtype=torch.uint8, device="cuda")
    bits_h = np.ones(100, np.uint8)
    out_h = np.full(4, 0xA5A5A5A5, np.uint32)
    out_d = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    assert L.nrLDPC_hip_codeword_scrambling(bits_d.data_ptr(), 100, 0, 1, 2, out_h.ctypes.data, 1, s) < 0
    assert "device memory" in hip.ldpc.last_error()
    assert L.nrLDPC_hip_codeword_scrambling(bits_h.ctypes.data, 100, 0, 1, 2, out_d.data_ptr(), 1, s) < 0
    llr_h = np.arange(100, dtype=np.int16)
    assert L.nrLDPC_hip_codeword_unscrambling(llr_h.ctypes.data, 100, 0, 1, 2, 1, s) < 0
    torch.cuda.synchronize()
    assert (out_h == 0xA5A5A5A5).all() and (out_d.cpu() == 7).all()
    assert np.array_equal(llr_h, np.arange(100, dtype=np.int16))
