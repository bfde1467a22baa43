"""The chain's first-transmission clear applied to the oracle's soft buffers -- test code only.

The reference clears d[r] over [0, Ncb) on round 0 (nr_rate_matching.c:554-555) and its decoder input reads whatever the
caller's buffer holds behind Ncb; the chain clears [0, max(Ncb, np(R))) instead, np(R) = ncols(R) Zc - 2 Zc being the
positions the round's rate mode R reads (nr_get_R_ldpc_decoder, uncut).  Rule R0: `clear_first_round` zeroes the part
[Ncb, np(R)) of each segment's oracle buffer before `oracle_lib.ulsch_decode(..., rnd=0)`; after that the oracle's
chain is the reference's and the GPU's soft values must equal it everywhere.  Rounds > 0 use the buffer as it is (R1):
nothing to apply."""
import oracle_lib as O


def ncb_of(tb, C_=None):
    """Ncb of the block's segments (nr_rate_matching.c:445-450)"""
    s = O.segmentation(None, O.len_with_crc(1, tb["A"]), tb["BG"])
    Cn = s["C"] if C_ is None else C_
    N = (66 if tb["BG"] == 1 else 50) * s["Z"]
    lbrm = tb.get("tbslbrm", 0)
    return N if not lbrm else min(N, 3 * lbrm // (2 * Cn))


def np_of(BG, Z, R):
    """soft-buffer positions the decoder reads in rate mode R"""
    return O.NCOLS[(BG, R)] * Z - 2 * Z


def clear_segment(d, ncb, BG, Z, R):
    """R0 on one segment's oracle buffer d (in place): zeros in [Ncb, np(R)), R the round's rate mode uncut"""
    np_ = np_of(BG, Z, R)
    if np_ > ncb:
        d[ncb:np_] = 0
    return d


def first_round_extents(tb, llrLen=0):
    """[(Ncb, np(R))] per segment for a round-0 call, R walked through the same stateful get_R / llrLen chain as
    oracle_lib.ulsch_decode; and the llrLen it leaves"""
    s = O.segmentation(None, O.len_with_crc(1, tb["A"]), tb["BG"])
    Z, Cn, BG = s["Z"], s["C"], tb["BG"]
    ncb = ncb_of(tb, Cn)
    out = []
    for r in range(Cn):
        E = O.get_E(tb["G"], Cn, tb["Qm"], tb["Nl"], r)
        R, llrLen = O.get_R(tb["rv"], E, BG, Z, llrLen, 0)
        out.append((ncb, np_of(BG, Z, R)))
    return out, llrLen


def clear_first_round(tb, harq_d, llrLen=0):
    """R0 on the oracle's buffers harq_d (one int16 array per segment, modified in place) ahead of a round-0 ulsch_decode;
    llrLen: the value that call starts from.  Returns the per-segment (Ncb, np(R))."""
    ext, _ = first_round_extents(tb, llrLen)
    for d, (ncb, np_) in zip(harq_d, ext):
        d[ncb:max(ncb, np_)] = 0
    return ext
