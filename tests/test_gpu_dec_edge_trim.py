"""-m gpu: the fast decoder's node bodies after one instruction per edge was taken out of both phases (ldpc_dec_fast_core.h: the
bit-node gather of the long columns sums the odd lanes as whole words, the check-node output bytes take their sign through two
three-input bit operations), against the oracle: full output rows and pass counts, numMaxIter 8.

Codes: BG1 Zc = 384 R = 1/3 (the lifting size's own instantiation: the degree-30 column, the degree-19 pair body, double tasks),
BG2 Zc = 384 R = 1/5 (other degrees, double tasks), BG1 Zc = 224 R = 1/3 (the general build with the stride in a register),
BG1 Zc = 8 and BG2 Zc = 16 with 32 blocks (several blocks per workgroup: ldpc_fast_bn with a block offset), BG1 Zc = 384 R = 8/9
(short columns, walked together, next to long ones).  Inputs: noise only (-12 dB, every pass runs), 1 dB (blocks stop early), and
the 1 dB words with random columns forced to +127 or -128 throughout, so that the bit-node sums reach both clamps."""
import numpy as np
import pytest

import oracle_lib as O
from common import make_llr

pytestmark = pytest.mark.gpu

CAP = 8
CASES = [(1, 384, 13, 8), (2, 384, 15, 8), (1, 224, 13, 8), (1, 8, 13, 32), (2, 16, 15, 32), (1, 384, 89, 8)]


def batch(BG, Z, R, n, kind, seed):
    rng = np.random.default_rng(seed)
    ncols = O.NCOLS[(BG, R)]
    rows = []
    for _ in range(n):
        llr = make_llr(rng, BG, Z, R, -12.0 if kind == "noise" else 1.0)[:ncols * Z].copy()
        if kind == "forced":      # a third of the columns, each wholly +127 or wholly -128
            for c in rng.choice(ncols, ncols // 3, replace=False):
                llr[c * Z:(c + 1) * Z] = 127 if rng.integers(2) else -128
        rows.append(llr)
    return np.ascontiguousarray(np.stack(rows), np.int8)


@pytest.mark.parametrize("kind", ["noise", "1dB", "forced"])
@pytest.mark.parametrize("BG,Z,R,n", CASES)
def test_rows_and_pass_counts_equal_the_oracle(hip, BG, Z, R, n, kind):
    llr = batch(BG, Z, R, n, kind, 9000 + 10 * Z + R + len(kind))
    ref = [O.decode(BG, Z, R, llr[i], CAP) for i in range(n)]
    its, outs = np.array([r[0] for r in ref], np.int32), np.stack([r[1] for r in ref])
    if kind == "noise":
        assert (its == CAP + 1).all(), its.tolist()        # every pass of every block runs
    if kind == "1dB":
        assert (its <= CAP).all(), its.tolist()            # every block stops early
    if kind == "forced":
        assert (np.abs(llr.astype(np.int32)) >= 127).any()
    # 2: the fast kernel or an error; 5: its several-blocks-per-workgroup form, which a launch this small would not pick itself
    n_iter, out = hip.decode_batch_host(BG, Z, R, llr, numMaxIter=CAP, kernel=5 if Z <= 64 else 2)
    print(BG, Z, R, kind, "passes (oracle):", its.tolist())
    assert np.array_equal(n_iter, its), (n_iter.tolist(), its.tolist())
    assert np.array_equal(out, outs)
