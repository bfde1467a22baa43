"""The DL-SCH / UL-SCH coding chain written from TS 38.212 alone: payload in, the G rate-matched bits out, and for the way back the
place of every one of those bits in the circular buffers.  It knows nothing of csrc/ and shares no line with oracle/, whose files
are near-transliterations of the reference: a misreading of the reference that the library and the oracle share does not pass it.
The one thing it takes from outside is oracle_lib.graph(BG, Zc, R), read as DATA: the entries of Tables 5.3.2-2 / 5.3.2-3 as (row,
column, V mod Zc), which test_tables.py pins against both copies the reference holds.  What is done with them is written here.

Clauses (38.212 unless 38.214 is named):

  5.1        gCRC24A, gCRC24B, gCRC16 from their polynomials: the remainder of a(D) D^L by g(D), bit-serial, register zero, parity
             appended MSB (p_0) first.
  7.2.1      L = 24 (CRC24A) if A > 3824, else 16.  Payload bytes carry a_0 in their most significant bit.
  7.2.2      the base graph is an input (38.214 chooses it).
  5.2.2      Kcb = 8448 / 3840; C = 1, L = 0 if B <= Kcb, else L = 24, C = ceil(B / (Kcb - L)); B' = B + C L; K' = B' / C; Kb = 22, or for
             base graph 2: 10 if B > 640, 9 if B > 560, 8 if B > 192, else 6; Zc the smallest of Table 5.3.2-1 with Kb Zc >= K'; K = 22
             Zc / 10 Zc; bits K' .. K - 1 are NULL; CRC24B over the K' - 24 bits of a block only when C > 1.
  5.3.2      fillers are 0 for the parity computation and NULL in d; d_k = c_(k + 2 Zc); H from the base graph with each 1 replaced by
             the identity shifted right by V mod Zc; w such that H [c w]^T = 0.
  5.4.2.1    Ncb = N, or min(N, N_ref), N_ref = floor(TBS_LBRM / (C R_LBRM)), R_LBRM = 2/3; E_r with C' = C; k0 of Table 5.4.2.1-2
             with the floor around num Ncb / (ncol Zc); e_k = d_((k0 + j) mod Ncb) for the j with d not NULL, in order.
  5.4.2.2    f_(i + j Qm) = e_(i E / Qm + j).
  5.5        the blocks' f back to back.

TBS_LBRM is an input (5.4.2.1 derives it from the configuration).  A transport block is the dict the library's calls take: A, G,
BG, Qm, Nl, rv, tbslbrm (0 = no limited buffer).

The standard has no receiver.  positions(tb) names, for each of the G bits, its segment and its index in that segment's circular
buffer; soft_buffers() is the plain sum of every LLR at its position, which is the only combining rule that follows from the
transmitter alone.

`mut` names ONE deliberate misreading (MUTATIONS below); the tests use it to show that their cases would notice it.  The default,
None, is the standard.
"""
import numpy as np

from oracle_lib import graph

NULL = -1

# Table 5.3.2-1, by set index i_LS
LIFTING = (
    (2, 4, 8, 16, 32, 64, 128, 256),
    (3, 6, 12, 24, 48, 96, 192, 384),
    (5, 10, 20, 40, 80, 160, 320),
    (7, 14, 28, 56, 112, 224),
    (9, 18, 36, 72, 144, 288),
    (11, 22, 44, 88, 176, 352),
    (13, 26, 52, 104, 208),
    (15, 30, 60, 120, 240),
)

# 5.1: the exponents of g(D) below D^L
G_CRC24A = (24, (23, 18, 17, 14, 11, 10, 7, 6, 5, 4, 3, 1, 0))
G_CRC24B = (24, (23, 6, 5, 1, 0))
G_CRC16 = (16, (12, 5, 0))

# Table 5.4.2.1-2: the numerators of k0 for rv 0 .. 3, and the denominator's column count
K0_NUM = {1: (0, 17, 33, 56), 2: (0, 13, 25, 43)}
NCOL = {1: 66, 2: 50}
KB_FULL = {1: 22, 2: 10}
KCB = {1: 8448, 2: 3840}
LOWEST_RATE = {1: 13, 2: 15}          # the name the table reader gives to the whole base graph

MUTATIONS = (
    ["k0 numerator + 1, BG%d rv%d" % (bg, rv) for bg in (1, 2) for rv in (0, 1, 2, 3)] + [
        "k0 not scaled by Ncb / N", "k0 floor after the multiplication by Zc", "wrap modulo N under LBRM",
        "N_ref: division by C before the 3/2", "E_r rule with <", "larger E first", "interleaver transposed", "fillers transmitted",
        "filler range one bit early", "CB CRC over the fillers too", "CRC24A for the code blocks", "CB CRC at C = 1", "A >= 3824",
        "Kb threshold 640 with >=", "Kb threshold 560 with >=", "Kb threshold 192 with >=", "Zc with Kb Zc > K'", "circulants shifted left",
        "payload bytes LSB first"])


def _is(mut, name):
    assert mut is None or mut in MUTATIONS, mut
    return mut == name


# ---- 5.1 ---------------------------------------------------------------------------------------------------------------------
def crc_parity(bits, g):
    """p_0 .. p_(L-1) for the bit sequence `bits` (0 / 1) and g = (L, exponents below D^L)"""
    L, taps = g
    poly = sum(1 << t for t in taps)
    top, mask = 1 << (L - 1), (1 << L) - 1
    reg = 0
    for b in np.asarray(bits, np.uint8).tolist():
        fb = ((reg & top) != 0) ^ b
        reg = (reg << 1) & mask
        if fb:
            reg ^= poly
    return np.array([(reg >> (L - 1 - i)) & 1 for i in range(L)], np.uint8)


def crc_attach(bits, g):
    bits = np.asarray(bits, np.uint8)
    return np.concatenate([bits, crc_parity(bits, g)])


# ---- 7.2.1 -------------------------------------------------------------------------------------------------------------------
def payload_bits(payload, A, mut=None):
    order = "little" if _is(mut, "payload bytes LSB first") else "big"
    return np.unpackbits(np.asarray(payload, np.uint8)[:(A + 7) // 8], bitorder=order)[:A]


def tb_crc_attach(a, mut=None):
    A = a.size
    big = A >= 3824 if _is(mut, "A >= 3824") else A > 3824
    return crc_attach(a, G_CRC24A if big else G_CRC16)


def tb_crc_len(A, mut=None):
    return 24 if (A >= 3824 if _is(mut, "A >= 3824") else A > 3824) else 16


# ---- 5.2.2 -------------------------------------------------------------------------------------------------------------------
def segment_sizes(B, BG, mut=None):
    """the numbers of 5.2.2 for B bits on base graph BG: dict(B, C, L, Bp, Kp, Kb, Zc, iLS, K, F, N, byte_contract).
    byte_contract: every block takes a whole number of payload bytes ((K' - L) % 8 == 0), which is what the library asks of a
    transport block beyond A % 8 == 0; every TBS of 38.214 5.1.3.2 meets it."""
    Kcb = KCB[BG]
    if B <= Kcb and not _is(mut, "CB CRC at C = 1"):
        L, C = 0, 1
    else:
        L = 24
        C = -(-B // (Kcb - L))
    Bp = B + C * L
    if Bp % C:
        raise ValueError("5.2.2 defines K' = B' / C only where C divides B'")
    Kp = Bp // C
    if BG == 1:
        Kb = 22
    else:
        ge = lambda t: B >= t if _is(mut, "Kb threshold %d with >=" % t) else B > t
        Kb = 10 if ge(640) else 9 if ge(560) else 8 if ge(192) else 6
    ok = (lambda z: Kb * z > Kp) if _is(mut, "Zc with Kb Zc > K'") else (lambda z: Kb * z >= Kp)
    cand = [(z, i) for i, row in enumerate(LIFTING) for z in row if ok(z)]
    if not cand:
        raise ValueError("no lifting size")
    Zc, iLS = min(cand)
    K = KB_FULL[BG] * Zc
    return dict(B=B, BG=BG, C=C, L=L, Bp=Bp, Kp=Kp, Kb=Kb, Zc=Zc, iLS=iLS, K=K, F=K - Kp, N=NCOL[BG] * Zc, byte_contract=(Kp - L) % 8 == 0)


def segment(b, BG, mut=None):
    """5.2.2: (sizes, [c_r]) with c_r int8[K], NULL at K' .. K - 1"""
    b = np.asarray(b, np.uint8)
    s = segment_sizes(b.size, BG, mut)
    out, pos = [], 0
    g = G_CRC24A if _is(mut, "CRC24A for the code blocks") else G_CRC24B
    for _ in range(s["C"]):
        c = np.full(s["K"], NULL, np.int8)
        n = s["Kp"] - s["L"]
        c[:n] = b[pos:pos + n]
        pos += n
        if s["L"]:
            over = np.concatenate([c[:n], np.zeros(s["F"], np.int8)]) if _is(mut, "CB CRC over the fillers too") else c[:n]
            c[n:s["Kp"]] = crc_parity(over.astype(np.uint8), g)
        out.append(c)
    assert pos == b.size
    return s, out


# ---- 5.3.2 -------------------------------------------------------------------------------------------------------------------
_GRAPHS = {}


def base_graph(BG, Zc):
    """[(row, column, V mod Zc)] of the whole base graph, and its (rows, columns)"""
    if (BG, Zc) not in _GRAPHS:
        g = graph(BG, Zc, LOWEST_RATE[BG])
        edges = [(r, int(g.col[e]), int(g.shift[e]) % Zc) for r in range(g.nrows) for e in range(g.row_ptr[r], g.row_ptr[r + 1])]
        assert g.ncols == NCOL[BG] + 2 and g.nrows == g.ncols - KB_FULL[BG]
        _GRAPHS[(BG, Zc)] = (edges, g.nrows, g.ncols)
    return _GRAPHS[(BG, Zc)]


def shifted(x, v, mut=None):
    """P x for P = the identity shifted right by v: row i of P has its 1 in column (i + v) mod Zc, so (P x)_i = x_((i + v) mod Zc)"""
    return np.roll(x, v if _is(mut, "circulants shifted left") else -v)


def syndrome(BG, Zc, word):
    """H word^T over GF(2) as one sparse product on H written out entry by entry: uint8[rows Zc].  word: the (ncols Zc) bits of c
    followed by w, fillers as 0."""
    edges, nrows, ncols = base_graph(BG, Zc)
    e = np.array(edges, np.int64)
    i = np.arange(Zc)
    rows = (e[:, 0, None] * Zc + i[None, :]).reshape(-1)
    cols = (e[:, 1, None] * Zc + (i[None, :] + e[:, 2, None]) % Zc).reshape(-1)
    s = np.zeros(nrows * Zc, np.int64)
    np.add.at(s, rows, np.asarray(word, np.int64)[cols])
    return (s & 1).astype(np.uint8)


def ldpc_encode(c, BG, Zc, mut=None):
    """5.3.2: c int8[K] with NULLs -> d int8[N] with NULLs.  The parity from the structure of H: the four core rows sum to one
    circulant times the first parity block; the other three core blocks follow by substitution; each extension row has a single
    identity in its own parity column."""
    edges, nrows, ncols = base_graph(BG, Zc)
    kb = KB_FULL[BG]
    c = np.asarray(c, np.int8)
    assert c.size == kb * Zc
    x = np.zeros((ncols, Zc), np.uint8)
    x[:kb] = np.where(c == NULL, 0, c).reshape(kb, Zc)
    by_row = [[(col, v) for r, col, v in edges if r == row] for row in range(nrows)]
    lam = np.zeros((nrows, Zc), np.uint8)                             # the information part of every row
    for row in range(nrows):
        for col, v in by_row[row]:
            if col < kb:
                lam[row] ^= shifted(x[col], v, mut)
    # first parity block: in the sum of the core rows the columns kb + 1 .. kb + 3 cancel (two identities each), and of the three
    # entries of column kb two have the same shift
    vs = [v for row in range(4) for col, v in by_row[row] if col == kb]
    left = [v for v in set(vs) if vs.count(v) % 2]
    assert len(left) == 1 and all(sum(1 for row in range(4) for col, _ in by_row[row] if col == kb + k) == 2 for k in (1, 2, 3))
    x[kb] = shifted(lam[0] ^ lam[1] ^ lam[2] ^ lam[3], (Zc - left[0]) % Zc, mut)
    known = set(range(kb + 1))
    while len(known) < kb + 4:                                        # a core row with one unknown block gives that block
        progress = False
        for row in range(4):
            unknown = [(col, v) for col, v in by_row[row] if col not in known]
            if len(unknown) == 1:
                col, v = unknown[0]
                acc = lam[row].copy()
                for c2, v2 in by_row[row]:
                    if kb <= c2 and c2 in known:
                        acc ^= shifted(x[c2], v2, mut)
                x[col] = shifted(acc, (Zc - v) % Zc, mut)
                known.add(col)
                progress = True
        assert progress
    for row in range(4, nrows):                                       # extension rows
        own = kb + row
        assert [(col, v) for col, v in by_row[row] if col >= kb + 4] == [(own, 0)]
        acc = lam[row].copy()
        for col, v in by_row[row]:
            if kb <= col < kb + 4:
                acc ^= shifted(x[col], v, mut)
        x[own] = acc
    word = x.reshape(-1)
    if mut is None:
        assert not syndrome(BG, Zc, word).any(), "the solve does not satisfy H"
    d = word[2 * Zc:].astype(np.int8)
    nul = np.flatnonzero(c == NULL)
    d[nul[nul >= 2 * Zc] - 2 * Zc] = NULL
    return d


# ---- 5.4.2.1 -----------------------------------------------------------------------------------------------------------------
def circular_buffer_len(N, C, tbslbrm, mut=None):
    if not tbslbrm:
        return N
    n_ref = (3 * (tbslbrm // C)) // 2 if _is(mut, "N_ref: division by C before the 3/2") else (3 * tbslbrm) // (2 * C)
    return min(N, n_ref)


def k0_of(BG, Zc, Ncb, rv, mut=None):
    num = K0_NUM[BG][rv] + (1 if _is(mut, "k0 numerator + 1, BG%d rv%d" % (BG, rv)) else 0)
    if _is(mut, "k0 not scaled by Ncb / N"):
        return num * Zc
    if _is(mut, "k0 floor after the multiplication by Zc"):
        return (num * Ncb * Zc) // (NCOL[BG] * Zc)
    return (num * Ncb) // (NCOL[BG] * Zc) * Zc


def block_sizes(G, C, Qm, Nl, mut=None):
    """E_r for r = 0 .. C - 1, every block transmitted (C' = C)"""
    q = G // (Nl * Qm)
    lo, hi = Nl * Qm * (q // C), Nl * Qm * (-(-q // C))
    out = []
    for r in range(C):
        first = r < C - q % C - 1 if _is(mut, "E_r rule with <") else r <= C - q % C - 1
        if _is(mut, "larger E first"):
            first = not (r <= q % C - 1)
        out.append(lo if first else hi)
    return out


def select(null, Ncb, k0, E, N, tbslbrm=0, mut=None):
    """the indices into d of e_0 .. e_(E-1): j = 0, 1, 2, ...; take (k0 + j) mod Ncb where d is not NULL"""
    null = np.asarray(null, bool)
    if _is(mut, "fillers transmitted"):
        null = np.zeros_like(null)
    if _is(mut, "filler range one bit early"):
        null = np.roll(null, -1)
    mod = N if (_is(mut, "wrap modulo N under LBRM") and tbslbrm) else Ncb
    good = int((~null[:mod]).sum())
    if good == 0:
        raise ValueError("nothing to transmit")
    laps = -(-E // good) + 1
    idx = (k0 + np.arange(laps * mod)) % mod
    idx = idx[~null[idx]]
    return idx[:E]


def interleave_index(E, Qm, mut=None):
    """p with f[k] = e[p[k]]"""
    i, j = np.meshgrid(np.arange(Qm), np.arange(E // Qm), indexing="ij")
    p = np.zeros(E, np.int64)
    if _is(mut, "interleaver transposed"):
        p[i * (E // Qm) + j] = i + j * Qm
    else:
        p[i + j * Qm] = i * (E // Qm) + j
    return p


def block_positions(BG, Zc, K, F, C, tbslbrm, rv, E, Qm, mut=None):
    """for one code block with F fillers at the end of its K bits: (the index in d of f_0 .. f_(E-1), Ncb, k0)"""
    N = NCOL[BG] * Zc
    null = np.zeros(N, bool)
    null[K - F - 2 * Zc:K - 2 * Zc] = True
    Ncb = circular_buffer_len(N, C, tbslbrm, mut)
    k0 = k0_of(BG, Zc, Ncb, rv, mut)
    return select(null, Ncb, k0, E, N, tbslbrm, mut)[interleave_index(E, Qm, mut)], Ncb, k0


# ---- the chain ---------------------------------------------------------------------------------------------------------------
def plan(tb, mut=None):
    """every number of a transport block's coding: the sizes of 5.2.2 plus A, Ltb, Ncb, k0, E (list), fs / fe (the filler range in
    d), V (transmittable positions of a lap)"""
    Ltb = tb_crc_len(tb["A"], mut)
    s = segment_sizes(tb["A"] + Ltb, tb["BG"], mut)
    Ncb = circular_buffer_len(s["N"], s["C"], tb.get("tbslbrm", 0), mut)
    fs, fe = s["Kp"] - 2 * s["Zc"], s["K"] - 2 * s["Zc"]
    V = Ncb - max(0, min(fe, Ncb) - min(fs, Ncb))
    return dict(s, A=tb["A"], Ltb=Ltb, Ncb=Ncb, k0=k0_of(tb["BG"], s["Zc"], Ncb, tb.get("rv", 0), mut),
                E=block_sizes(tb["G"], s["C"], tb["Qm"], tb["Nl"], mut), fs=fs, fe=fe, V=V)


def code_blocks(tb, payload, mut=None):
    """(plan, [d_r]) : 7.2.1, 5.2.2, 5.3.2"""
    a = payload_bits(payload, tb["A"], mut)
    s, cs = segment(tb_crc_attach(a, mut), tb["BG"], mut)
    return s, [ldpc_encode(c, tb["BG"], s["Zc"], mut) for c in cs]


def positions(tb, mut=None):
    """(segment int32[G], index in that segment's circular buffer int32[G]) of the G output bits"""
    p = plan(tb, mut)
    seg, idx = [], []
    for r, E in enumerate(p["E"]):
        i, _, _ = block_positions(tb["BG"], p["Zc"], p["K"], p["F"], p["C"], tb.get("tbslbrm", 0), tb.get("rv", 0), E, tb["Qm"], mut)
        seg.append(np.full(E, r, np.int32))
        idx.append(i.astype(np.int32))
    return np.concatenate(seg), np.concatenate(idx)


def dlsch(tb, payload, mut=None):
    """uint8[G], one bit per byte"""
    _, ds = code_blocks(tb, payload, mut)
    seg, idx = positions(tb, mut)
    out = np.stack(ds)[seg, idx]
    if _is(mut, "fillers transmitted") or _is(mut, "filler range one bit early"):
        out = np.where(out == NULL, 0, out)
    assert (out != NULL).all() and out.size == tb["G"]
    return out.astype(np.uint8)


def soft_buffers(tb_rounds, llrs, start=None):
    """[int16[Ncb]] per segment after the given rounds: tb_rounds = the transport block's dict once per round (rv and G may change,
    the rest may not), llrs = int16[G] per round.  start=None: the first round is round 0 and zeros the buffers; otherwise start =
    the buffers' contents before the first of the given rounds.  Every LLR is added at its position; fillers are never touched."""
    p0 = plan(tb_rounds[0])
    if start is None:
        buf = [np.zeros(p0["Ncb"], np.int64) for _ in range(p0["C"])]
    else:
        buf = [np.asarray(b, np.int64)[:p0["Ncb"]].copy() for b in start]
    for tb, llr in zip(tb_rounds, llrs):
        p = plan(tb)
        assert (p["C"], p["Ncb"], p["Zc"]) == (p0["C"], p0["Ncb"], p0["Zc"])
        seg, idx = positions(tb)
        for r in range(p["C"]):
            np.add.at(buf[r], idx[seg == r], np.asarray(llr, np.int64)[seg == r])
    assert all(np.abs(b).max(initial=0) <= 32767 for b in buf), "the inputs leave int16: the model has no rule for that"
    return [b.astype(np.int16) for b in buf]
