"""-m gpu: the fast batch decoder outside its passes -- prologue with the LLR extents in the kernel arguments and unconditional LLR
loads, hard decision, and (builds with -DLDPC_DEC_WARM=1) the next row warmed in L2 (ldpc_dec_fast_block.h) -- through
decode_batch_device against the oracle, at the batch sizes where the index blockIdx.x + (resident workgroups) falls inside, on and
past the end of the batch: 1, 3, n_cus - 1, n_cus + 1 and 2 n_cus + 5 blocks.  Codes: dec_block_ends_inputs.CODES.  kernel = 3: the
one-block-per-workgroup kernel in its throughput shape, which a batch this small of a small code would not get by itself.

The LLR tensor is exactly n rows of num_llr bytes, so it ends with the last row: a load past the end of the batch would leave the
allocation.  The blocks are the three rows of stop_rows (pass counts 3, 4, numMaxIter + 1 by the oracle) repeated, the output
tensor is prefilled with 0xAA and four guard bytes lie on both sides of every row; one case has the whole output tensor 4 bytes
behind a 16-byte boundary."""
import numpy as np
import pytest

from dec_block_ends_inputs import CAP, CODES, stop_rows

pytestmark = pytest.mark.gpu


def sizes(hip):
    import torch
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    return [1, 3, n_cus - 1, n_cus + 1, 2 * n_cus + 5]


def check(hip, BG, Z, R, n, out_offset=0):
    import torch
    llr3, its3, outs3 = stop_rows(BG, Z, R)
    idx = np.arange(n) % 3
    ob = outs3.shape[1]
    llr = torch.from_numpy(np.ascontiguousarray(llr3[idx])).cuda()
    assert llr.is_contiguous() and llr.shape == (n, llr3.shape[1])        # ends with the last row
    pitch = ob + 8
    raw = torch.full((32 + n * pitch,), 0xAA, dtype=torch.uint8, device="cuda")
    base = (-raw.data_ptr()) % 16 + out_offset                              # 16-byte aligned, or 4 bytes behind that
    rows = raw[base:base + n * pitch].view(n, pitch)
    out = rows[:, 4:4 + ob]
    assert out.data_ptr() % 4 == 0 and (out.data_ptr() - 4) % 16 == out_offset
    it = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    hip.decode_batch_device(BG, Z, R, llr, out, it, numMaxIter=CAP, kernel=3)
    torch.cuda.synchronize()
    assert np.array_equal(it.cpu().numpy(), its3[idx]), (BG, Z, R, n)
    got = rows.cpu().numpy()
    assert np.array_equal(got[:, 4:4 + ob], outs3[idx]), (BG, Z, R, n, np.flatnonzero((got[:, 4:4 + ob] != outs3[idx]).any(axis=1))[:8].tolist())
    assert (got[:, :4] == 0xAA).all() and (got[:, 4 + ob:] == 0xAA).all()
    rest = raw.cpu().numpy()
    assert (rest[:base] == 0xAA).all() and (rest[base + n * pitch:] == 0xAA).all()


@pytest.mark.parametrize("BG,Z,R", CODES)
def test_rows_and_pass_counts_at_the_batch_sizes_around_one_round(hip, BG, Z, R):
    for n in sizes(hip):
        check(hip, BG, Z, R, n)


def test_output_tensor_four_bytes_behind_a_16_byte_boundary(hip):
    for BG, Z, R in (CODES[0], CODES[5]):
        for n in sizes(hip)[1:4]:
            check(hip, BG, Z, R, n, out_offset=4)
