"""The Gold sequence of 38.211 5.2.1 as the library generates it (nr_gold.h through the host entry point
nrLDPC_hip_gold_words, no GPU): word-level jump-ahead against a bit-serial restatement of the definition, the known-answer
words, and argument checks of every scrambling entry point (they fail before touching a GPU)."""
import ctypes as C

import numpy as np
import pytest

NC = 1600


def serial_gold(c_init, n_bits):
    """c(0 .. n_bits-1), bit by bit as 38.211 5.2.1 states it: c(n) = x1(n + Nc) ^ x2(n + Nc),
    x1(n + 31) = x1(n + 3) ^ x1(n), x2(n + 31) = x2(n + 3) ^ x2(n + 2) ^ x2(n + 1) ^ x2(n),
    x1(0) = 1, x1(1..30) = 0, x2(0..30) = the bits of c_init."""
    n = NC + n_bits
    x1 = np.zeros(n, np.uint8)
    x2 = np.zeros(n, np.uint8)
    x1[0] = 1
    x2[:31] = [(c_init >> i) & 1 for i in range(31)]
    # 28 new bits at a time: the nearest tap of x(n + 31) is x(n + 3), 28 bits back, so every tap of a block is known
    for s in range(0, n - 31, 28):
        e = min(s + 28, n - 31)
        x1[s + 31:e + 31] = x1[s + 3:e + 3] ^ x1[s:e]
    for s in range(0, n - 31, 28):
        e = min(s + 28, n - 31)
        x2[s + 31:e + 31] = x2[s + 3:e + 3] ^ x2[s + 2:e + 2] ^ x2[s + 1:e + 1] ^ x2[s:e]
    return x1[NC:] ^ x2[NC:]


def words_of(bits):
    """bit k of word w = bits[32 w + k]"""
    b = bits.reshape(-1, 32).astype(np.uint64)
    return (b << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def c_init_of(n_rnti, q, n_id):
    return (n_rnti << 15) + (q << 14) + n_id


C_INITS = [0, c_init_of(0, 1, 0), c_init_of(0xFFFF, 0, 0), c_init_of(0, 0, 1023), c_init_of(0xFFFF, 1, 1023),
           c_init_of(0x4601, 0, 17), 0x7FFFFFFF]


@pytest.fixture(scope="module")
def ldpc(built):
    import openairinterface5g_amd as pkg
    return pkg.ldpc


@pytest.fixture(scope="module")
def spec():
    """the first 65 700 words of the sequence for every c_init above, bit-serially"""
    return {ci: words_of(serial_gold(ci, 32 * (65536 + 164))) for ci in C_INITS}


def test_known_answer_words(ldpc):
    ci = c_init_of(0xFFFF, 1, 1023)
    assert [f"{w:08x}" for w in ldpc.gold_words(ci, 0, 6)] == \
        ["73594600", "307f5338", "96c05d5b", "efeeabde", "e1e22736", "cc33d149"]


@pytest.mark.parametrize("c_init", C_INITS)
def test_jump_ahead_matches_the_bit_serial_definition(ldpc, spec, c_init):
    ref = spec[c_init]
    for first in (0, 1, 31, 32, 63, 64, 65535):
        for n in (1, 3, 65, 100):
            assert np.array_equal(ldpc.gold_words(c_init, first, n), ref[first:first + n]), (first, n)


def test_random_offsets_and_lengths(ldpc, spec):
    rng = np.random.default_rng(7)
    for _ in range(200):
        ci = C_INITS[int(rng.integers(len(C_INITS)))]
        first = int(rng.integers(0, 65536))
        n = int(rng.integers(1, 130))
        assert np.array_equal(ldpc.gold_words(ci, first, n), spec[ci][first:first + n]), (ci, first, n)


def test_a_long_run_from_word_zero(ldpc, spec):
    ci = c_init_of(0x1234, 1, 511)
    ref = words_of(serial_gold(ci, 32 * 7681))
    assert np.array_equal(ldpc.gold_words(ci, 0, 7681), ref)  # ceil(245 700 / 32): one transport block of the 64-TB slot


def test_gold_words_argument_checks(ldpc):
    L = ldpc._scr_lib()
    out = np.full(4, 0xA5A5A5A5, np.uint32)
    assert L.nrLDPC_hip_gold_words(1 << 31, 0, 4, out.ctypes.data) < 0          # c_init has 31 bits
    assert "c_init" in ldpc.last_error()
    assert L.nrLDPC_hip_gold_words(5, (1 << 17) - 50, 4, out.ctypes.data) < 0   # beyond the jump tables
    assert "first_word" in ldpc.last_error()
    assert L.nrLDPC_hip_gold_words(5, 0, 4, None) < 0
    assert (out == 0xA5A5A5A5).all()
    assert L.nrLDPC_hip_gold_words(5, (1 << 17) - 51, 4, out.ctypes.data) == 0  # the last first_word the tables reach
    assert L.nrLDPC_hip_gold_words(5, 0, 0, None) == 0


@pytest.mark.parametrize("n_rnti,q,n_id,what", [(0x10000, 0, 0, "n_RNTI"), (0, 2, 0, "q"), (0, 0, 1024, "n_ID")])
def test_scrambling_calls_reject_bad_parameters_before_any_work(ldpc, n_rnti, q, n_id, what):
    """validation comes first: these return without a GPU, and nothing is written"""
    L = ldpc._scr_lib()
    bits = np.ones(100, np.uint8)
    out = np.full(4, 0xA5A5A5A5, np.uint32)
    assert L.nrLDPC_hip_codeword_scrambling(bits.ctypes.data, 100, q, n_id, n_rnti, out.ctypes.data, 0, None) < 0
    assert what in ldpc.last_error()
    assert (out == 0xA5A5A5A5).all()
    llr = np.arange(100, dtype=np.int16)
    assert L.nrLDPC_hip_codeword_unscrambling(llr.ctypes.data, 100, q, n_id, n_rnti, 0, None) < 0
    assert what in ldpc.last_error()
    assert np.array_equal(llr, np.arange(100, dtype=np.int16))


def test_scrambling_calls_reject_bad_mem_size_and_pointers(ldpc):
    L = ldpc._scr_lib()
    bits = np.ones(64, np.uint8)
    out = np.zeros(2, np.uint32)
    assert L.nrLDPC_hip_codeword_scrambling(bits.ctypes.data, 64, 0, 1, 2, out.ctypes.data, 7, None) < 0
    assert "mem" in ldpc.last_error()
    assert L.nrLDPC_hip_codeword_scrambling(bits.ctypes.data, (1 << 21) + 1, 0, 1, 2, out.ctypes.data, 0, None) < 0
    assert L.nrLDPC_hip_codeword_scrambling(None, 64, 0, 1, 2, out.ctypes.data, 0, None) < 0
    assert L.nrLDPC_hip_codeword_scrambling(bits.ctypes.data, 64, 0, 1, 2, None, 0, None) < 0
    assert L.nrLDPC_hip_codeword_unscrambling(None, 64, 0, 1, 2, 0, None) < 0
    assert L.nrLDPC_hip_codeword_unscrambling(C.c_void_p(bits.ctypes.data), 64, 0, 1, 2, 3, None) < 0
    assert (out == 0).all()


def test_python_wrappers_refuse_a_size_beyond_the_array(ldpc):
    """the size a caller names is checked against the array before the library is called: no read or write behind it"""
    bits = np.ones(100, np.uint8)
    with pytest.raises(ValueError):
        ldpc.codeword_scrambling(bits, 0, 1, 2, size=101)
    llr = np.arange(100, dtype=np.int16)
    with pytest.raises(ValueError):
        ldpc.codeword_unscrambling(llr, 0, 1, 2, size=101)
    with pytest.raises(ValueError):
        ldpc.codeword_unscrambling(llr, 0, 1, 2, size=-1)
    assert np.array_equal(llr, np.arange(100, dtype=np.int16))
