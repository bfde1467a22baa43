"""A float64 PDSCH transmitter written from TS 38.211 / 38.214 alone: coded bits in, the transmit grid of every antenna port out.
It knows nothing of csrc/ and shares no line with the restatements of the reference that the other DL tests compare the library
with: its Gold sequence, its constellations, its layer mapping, its DMRS tables and its mapping are written here from the clauses
named below, so a misreading of the reference that the library and its restatements share does not pass it.  test_dl_slot_host.py
holds the CPU forms of the library to it within a bound derived from the library's arithmetic and shows that the comparison would
notice each of a list of small mistakes; test_gpu_dl_slot.py holds the GPU to the same bound on the same CASES.

What the model computes (38.211 unless 38.214 is named):

  5.2.1      c(n) = x1(n + Nc) + x2(n + Nc) mod 2, Nc = 1600, x1(n + 31) = x1(n + 3) + x1(n), x2(n + 31) = x2(n + 3) + x2(n + 2) +
             x2(n + 1) + x2(n), x1 = 1, 0, 0, ..., x2(0..30) = the bits of c_init.
  7.3.1.1    b~(i) = b(i) + c(i) mod 2 with c_init = n_RNTI 2^15 + q 2^14 + n_ID.
  5.1.3-6    QPSK, 16QAM, 64QAM, 256QAM in closed form; unit mean power each.
  7.3.1.3    one codeword on v = 1..4 layers: x^(l)(i) = d(v i + l).
  7.4.1.1.1  r(n) = ((1 - 2 c(2n)) + j (1 - 2 c(2n + 1))) / sqrt 2, c_init = (2^17 (14 n_s + l + 1)(2 N_ID + 1) + 2 N_ID + n_SCID) mod
             2^31 (the Release 15 form: no lambda-bar term).
  7.4.1.1.2  a(k, l) = beta w_f(k') w_t(l') r(2n + k'), k = 4n + 2k' + Delta (type 1) or 6n + k' + Delta (type 2), k' = 0, 1, l = l-bar +
             l'.  k counts from subcarrier 0 of CRB 0; for a PDSCH scheduled with SI-RNTI from subcarrier 0 of the lowest RB of
             CORESET 0, which is where the initial BWP starts: the BWP's own start is left out of k.  Tables 7.4.1.1.2-1 and -2 are
             typed below row by row.  l' = 0 on the first and 1 on the second symbol of each pair of adjacent DMRS symbols, read from
             the whole slot's bitmap, not from the allocated symbols.
  7.3.1.5/6  the layers' symbols go to the REs of the allocated VRBs that are not used for DMRS and do not belong to a CDM group
             without data (38.214 5.1.6.2: groups 0 .. ncdm - 1), in increasing order of first k, then l; non-interleaved, VRB n =
             PRB n of the BWP.  Grid subcarrier (first_carrier_offset + 12 (bwp_start + rb_start) + i) mod N.
  ports      layer l is sent on the l-th port of the set `dmrs_ports` (a bitmap over 1000 + bit); an empty set means port 1000.
  beta_DMRS  a parameter.  38.214 Table 4.1-1 gives sqrt(ncdm) (0, 3, 4.77 dB for 1, 2, 3 groups without data).
  precoding  antenna a of an RE is sum_l W[l][a] x_l, pilots and data alike (38.214 5.1.2.3: the DMRS is precoded as the data of its
             PRG is).  PMI 0 is layer a on antenna a and nothing behind the layers.  Which PRG an RB belongs to is a parameter:
             prg_origin = "crb": 38.214 5.1.2.3, the PRGs partition the BWP in units of P' RBs counted from CRB 0, so the first PRG of an
             allocation is partial unless bwp_start + rb_start is a multiple of P'; "allocation": PRG q is RBs q P' .. q P' + P' - 1 of
             the allocation, whatever its first RB.

The output is complex128 [n_ant, 14, N] with unit average symbol power on a layer (a pilot has modulus beta) and a boolean mask [14,
N] of the REs of the allocation: every antenna is defined there (0 on the REs of other CDM groups and behind the layers), nothing
is said about the rest.
"""
import numpy as np

NC = 1600

# Table 7.4.1.1.2-1 (configuration type 1): p - 1000, CDM group, Delta, w_f(0), w_f(1), w_t(0), w_t(1)
TABLE_TYPE1 = (
    (0, 0, 0, +1, +1, +1, +1),
    (1, 0, 0, +1, -1, +1, +1),
    (2, 1, 1, +1, +1, +1, +1),
    (3, 1, 1, +1, -1, +1, +1),
    (4, 0, 0, +1, +1, +1, -1),
    (5, 0, 0, +1, -1, +1, -1),
    (6, 1, 1, +1, +1, +1, -1),
    (7, 1, 1, +1, -1, +1, -1),
)
# Table 7.4.1.1.2-2 (configuration type 2)
TABLE_TYPE2 = (
    (0, 0, 0, +1, +1, +1, +1),
    (1, 0, 0, +1, -1, +1, +1),
    (2, 1, 2, +1, +1, +1, +1),
    (3, 1, 2, +1, -1, +1, +1),
    (4, 2, 4, +1, +1, +1, +1),
    (5, 2, 4, +1, -1, +1, +1),
    (6, 0, 0, +1, +1, +1, -1),
    (7, 0, 0, +1, -1, +1, -1),
    (8, 1, 2, +1, +1, +1, -1),
    (9, 1, 2, +1, -1, +1, -1),
    (10, 2, 4, +1, +1, +1, -1),
    (11, 2, 4, +1, -1, +1, -1),
)


def dmrs_table(dmrs_type):
    """dmrs_type as in the PDU: 0 = configuration type 1, 1 = configuration type 2"""
    return TABLE_TYPE2 if dmrs_type else TABLE_TYPE1


def gold(c_init, n):
    """c(0 .. n - 1) of 5.2.1 as uint8"""
    total = NC + n
    x1 = np.zeros(total + 31, np.uint8)
    x2 = np.zeros(total + 31, np.uint8)
    x1[0] = 1
    for i in range(31):
        x2[i] = (c_init >> i) & 1
    for i in range(total):
        x1[i + 31] = x1[i + 3] ^ x1[i]
        x2[i + 31] = x2[i + 3] ^ x2[i + 2] ^ x2[i + 1] ^ x2[i]
    return x1[NC:NC + n] ^ x2[NC:NC + n]


def scramble(bits, n_rnti, q, n_id):
    """7.3.1.1"""
    b = np.asarray(bits, np.uint8) & 1
    return b ^ gold(n_rnti * 2 ** 15 + q * 2 ** 14 + n_id, b.size)


def modulate(bits, Qm):
    """5.1.3 - 5.1.6: b(Qm i) .. b(Qm i + Qm - 1) -> d(i)"""
    s = 1 - 2 * np.asarray(bits, np.int64).reshape(-1, Qm)          # s[:, k] = 1 - 2 b(Qm i + k)
    if Qm == 2:
        re, im, norm = s[:, 0], s[:, 1], 2.0
    elif Qm == 4:
        re, im, norm = s[:, 0] * (2 - s[:, 2]), s[:, 1] * (2 - s[:, 3]), 10.0
    elif Qm == 6:
        re, im, norm = s[:, 0] * (4 - s[:, 2] * (2 - s[:, 4])), s[:, 1] * (4 - s[:, 3] * (2 - s[:, 5])), 42.0
    elif Qm == 8:
        re = s[:, 0] * (8 - s[:, 2] * (4 - s[:, 4] * (2 - s[:, 6])))
        im = s[:, 1] * (8 - s[:, 3] * (4 - s[:, 5] * (2 - s[:, 7])))
        norm = 170.0
    else:
        raise ValueError("Qm must be 2, 4, 6 or 8")
    return (re + 1j * im) / np.sqrt(norm)


def to_layers(d, v):
    """7.3.1.3, one codeword: complex [v, M / v]"""
    assert d.size % v == 0
    return np.stack([d[l::v] for l in range(v)])


def ports_of(dmrs_ports, v):
    """the l-th member of the port set for layer l; the empty set is port 1000"""
    if dmrs_ports == 0:
        return [0] * v
    members = [p for p in range(12) if dmrs_ports & (1 << p)]
    assert len(members) >= v, "fewer ports than layers"
    return members[:v]


def l_primes(symb_pos):
    """{l: l'} over the DMRS symbols of the slot: the second symbol of a pair of adjacent ones has l' = 1"""
    out = {}
    for l in range(14):
        if symb_pos & (1 << l):
            out[l] = 1 if out.get(l - 1) == 0 else 0
    return out


def dmrs_c_init(n_s, l, n_id, n_scid):
    return (2 ** 17 * (14 * n_s + l + 1) * (2 * n_id + 1) + 2 * n_id + n_scid) % 2 ** 31


def prg_of_rb(rb, first_crb, prg_size, prg_origin):
    """the index, among the PRGs that the allocation touches, of the PRG of the allocation's RB `rb`"""
    if prg_origin == "allocation":
        return rb // prg_size
    assert prg_origin == "crb"
    return (first_crb + rb) // prg_size - first_crb // prg_size


def pdsch_grid(p, bits, n_ant, beta_dmrs=1.0, prg_size=0, pmis=(), matrices=None, prg_origin="allocation"):
    """p: Nl, Qm, rnti, q, n_id (7.3.1.1), dmrs_config_type, num_dmrs_cdm_grps_no_data, dmrs_ports, scid, dl_dmrs_scrambling_id,
    slot, si_rnti, fft_size, first_carrier_offset, bwp_start, rb_start, rb_size, start_symbol, nr_of_symbols, dl_dmrs_symb_pos.
    bits: the codeword.  prg_size 0: no precoding (PMI 0 everywhere); else pmis[q] is the PMI of the allocation's q-th PRG and
    matrices[pmi] a complex array [Nl, n_ant].  Returns (grid complex128 [n_ant, 14, N], mask bool [14, N])."""
    v, Qm, N, typ, ncdm = p["Nl"], p["Qm"], p["fft_size"], p["dmrs_config_type"], p["num_dmrs_cdm_grps_no_data"]
    x = to_layers(modulate(scramble(bits, p["rnti"], p["q"], p["n_id"]), Qm), v)
    rows = [dmrs_table(typ)[port] for port in ports_of(p["dmrs_ports"], v)]
    comb = 2 if typ == 0 else 6                                         # a CDM group is Delta, Delta + 1 mod 6 (type 2) or Delta mod 2 (type 1)
    width = 1 if typ == 0 else 2
    first_crb = p["bwp_start"] + p["rb_start"]
    ref_rb = p["rb_start"] if p["si_rnti"] else first_crb              # the allocation's first RB counted from the reference point of k
    lp = l_primes(p["dl_dmrs_symb_pos"])
    n_sc = 12 * p["rb_size"]
    layer_grid = np.zeros((v, 14, n_sc), np.complex128)                # on the allocation's subcarriers i = 0 .. n_sc - 1
    taken = np.zeros(v, np.int64)
    for l in range(p["start_symbol"], p["start_symbol"] + p["nr_of_symbols"]):
        if l in lp:
            k_abs = 12 * ref_rb + np.arange(n_sc)                       # k of 7.4.1.1.2 for each allocated subcarrier
            c = gold(dmrs_c_init(p["slot"], l, p["dl_dmrs_scrambling_id"], p["scid"]), 2 * (int(k_abs[-1]) + 2))
            r = ((1 - 2.0 * c[0::2]) + 1j * (1 - 2.0 * c[1::2])) / np.sqrt(2.0)
            no_data = np.zeros(n_sc, bool)
            for g in range(ncdm):                                       # the REs of CDM groups 0 .. ncdm - 1 carry no PDSCH
                delta_g = g if typ == 0 else 2 * g
                no_data |= (k_abs - delta_g) % comb < width
            for j, (port, group, delta, wf0, wf1, wt0, wt1) in enumerate(rows):
                wt = (wt0, wt1)[lp[l]]
                pilot = (k_abs - delta) % comb < width
                for i in np.flatnonzero(pilot):
                    k = int(k_abs[i]) - delta
                    n, kp = (k // 4, (k // 2) % 2) if typ == 0 else (k // 6, k % 6)
                    layer_grid[j, l, i] = beta_dmrs * (wf0, wf1)[kp] * wt * r[2 * n + kp]
                data = ~(no_data | pilot)
                cnt = int(data.sum())
                layer_grid[j, l, data] = x[j, taken[j]:taken[j] + cnt]
                taken[j] += cnt
        else:
            for j in range(v):
                layer_grid[j, l] = x[j, taken[j]:taken[j] + n_sc]
                taken[j] += n_sc
    assert (taken == x.shape[1]).all(), "the codeword does not fill the allocation exactly"
    # antenna ports
    ant_grid = np.zeros((n_ant, 14, n_sc), np.complex128)
    for rb in range(p["rb_size"]):
        pmi = pmis[prg_of_rb(rb, first_crb, prg_size, prg_origin)] if prg_size else 0
        sl = slice(12 * rb, 12 * rb + 12)
        if pmi == 0:
            ant_grid[:min(v, n_ant), :, sl] = layer_grid[:min(v, n_ant), :, sl]
        else:
            W = np.asarray(matrices[pmi], np.complex128)
            assert W.shape == (v, n_ant)
            ant_grid[:, :, sl] = np.einsum("la,lsk->ask", W, layer_grid[:, :, sl])
    grid = np.zeros((n_ant, 14, N), np.complex128)
    mask = np.zeros((14, N), bool)
    k_grid = (p["first_carrier_offset"] + 12 * first_crb + np.arange(n_sc)) % N
    syms = np.arange(p["start_symbol"], p["start_symbol"] + p["nr_of_symbols"])
    grid[:, syms[:, None], k_grid[None, :]] = ant_grid[:, syms]
    mask[syms[:, None], k_grid[None, :]] = True
    return grid, mask


# ---- the slots ---------------------------------------------------------------------------------------------------------------
def _case(name, Nl, n_tx, typ, ports, ncdm, pos, Qm, amp, N, rb, first_rb, start=0, n_sym=14, si=0, prg=None, pmis=(), BG=2):
    return dict(name=name, Nl=Nl, n_tx=n_tx, typ=typ, ports=ports, ncdm=ncdm, pos=pos, Qm=Qm, amp=amp, N=N, rb=rb, first_rb=first_rb, start=start,
                n_sym=n_sym, si=si, prg=prg, pmis=list(pmis), BG=BG)


# first_rb = (bwp_start, rb_start): their sum is odd and not zero in every case, and every allocation runs over the end of the grid
# (test_dl_slot_host.py places it and asserts both).  prg: None = the unit call; else prg_size, with pmis one per PRG.
CASES = [
    _case("1", 1, 1, 0, 0b1, 1, 1 << 2, 2, 512, 128, 2, (2, 1)),
    _case("2", 1, 2, 0, 0b10, 1, 1 << 3, 4, 8192, 256, 3, (4, 3)),
    _case("3", 2, 3, 0, 0b1100, 2, 0b11 << 2, 6, 32767, 256, 4, (1, 4)),
    _case("4", 4, 4, 0, 0b10100101, 2, 0b11 << 2, 4, 512, 512, 5, (6, 5)),
    _case("5", 4, 5, 1, 0b110000001100, 3, 0b11 << 3, 8, 8192, 256, 3, (0, 7)),
    _case("6", 2, 2, 1, 0b11, 1, 1 << 2 | 1 << 7 | 1 << 11, 4, 32767, 128, 2, (8, 1)),
    _case("7", 1, 1, 0, 0, 2, 1 << 2, 2, 8192, 256, 6, (7, 2), start=2, n_sym=6, si=1),
    _case("8", 1, 1, 1, 0b10, 1, 0b11 << 2, 4, 512, 128, 4, (3, 2), start=3, n_sym=5),
    _case("9", 2, 4, 0, 0b11, 1, 1 << 2, 6, 8192, 512, 5, (2, 3), prg=2, pmis=(1, 0, 2)),
    _case("10", 4, 8, 1, 0b11000011, 2, 0b11 << 2, 4, 32767, 256, 3, (5, 4), prg=3, pmis=(3,)),
    _case("11", 1, 2, 0, 0b1, 1, 1 << 2, 2, 512, 256, 6, (4, 3), prg=4, pmis=(1, 2)),
    _case("12", 3, 3, 1, 0b111, 2, 1 << 3, 6, 8192, 128, 2, (1, 2)),   # three layers, which none of the eleven above has
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
