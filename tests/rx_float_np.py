"""A float64 model of the three UL receivers, written from textbook detection and the constellations of TS 38.211 5.1 -- not from
csrc/, not from the reference's source and not from the numpy restatements (rx_front_np.py, qam_np.py, rx_mmse_np.py, rx_ml_np.py),
none of which it imports.  It takes the int16 rx [n_rx, nb_re, 2] and ch ([n_rx, nb_re, 2], or [2, n_rx, nb_re, 2] for two layers)
the receivers take, as complex128, and returns what the receiver's int16 output would be without any rounding: float64 LLRs in
LSB of the output.  The power-of-two and amplitude factors that bring a textbook quantity to that LSB are derived here from what
the interface documents (the shift, the Q15 amplitudes, the output's order), never fitted.

The model of the link: r[a] = sum_l h[l, a] x[l] + n, x a point of the unit-power constellation of 38.211 5.1.2 .. 5.1.5,
    d = ((1 - 2 b0) A(b2, b4, b6) + j (1 - 2 b1) A(b3, b5, b7)) / sqrt(norm),
    A = 1 (QPSK), 2 - (1 - 2 b) (16QAM), 4 - (1 - 2 b)(2 - (1 - 2 b')) (64QAM), 8 - (1 - 2 b)(4 - (1 - 2 b')(2 - (1 - 2 b''))) (256QAM),
    norm = 2, 10, 42, 170.  An LLR is positive where the bit is more likely 0.

Single layer.  z = sum_a conj(h[a]) r[a] = E x + noise with E = sum_a |h[a]|^2.  Per dimension v = Re z or Im z the max-log LLRs
of the nested constellation are, to the usual nested-distance approximation, L0 = v, L1 = 2^(Qm/2 - 1) E / sqrt(norm) - |L0|,
L2 = 2^(Qm/2 - 2) E / sqrt(norm) - |L1|, ...: each level folds the axis at the middle of the remaining points.  The receiver shifts
every product right by `shift` before it adds, so its output is 2^-shift of that; its magnitudes are E 2^-shift times the Q15
constants round(2^15 2^(Qm/2 - k) / sqrt(norm)) / 2^15, which is the same factor.  QPSK has no magnitude and its LLR is the
compensated value shifted right by 3 more: 2^-(shift + 3).  Order per RE: L0(Re), L0(Im), L1(Re), L1(Im), ... = bits b0, b1, b2, ...

Two-layer MMSE (64QAM, 256QAM).  xhat = (H^H H + lambda I)^-1 H^H r through numpy.linalg.solve.  The receiver forms G = (H^H H)
2^-shift and adds nvar to G's diagonal after that shift, so lambda = nvar 2^shift.  It then multiplies by the adjugate instead of
dividing: its equalised value is det(G) xhat 2^-b and its magnitude unit det(G) 2^-b, where b = floor(log2(sum over the four REs
of a quad of floor(det(G) / 4))) + 1 - 8 brings the quad's mean determinant to 128 .. 255; the REs behind a segment's last one
count as zero channels (det = nvar^2).  With K = det(G) 2^-b the LLRs are the single-layer demapper's on v = K xhat with unit K.

Two-layer ML (QPSK, 16QAM).  LLR of bit k of layer d = max over the candidate pairs with the bit 0 of M - max over those with
the bit 1, M = -|r - h0 x0 - h1 x1|^2 (ml_exhaustive).  Expanded, with z_l = h_l^H r, E_l = |h_l|^2 and rho_id = h_i^H h_d,
    M + |r|^2 = 2 Re(xd* z_d) - |xd|^2 E_d + [2 Re(xi* (z_i - rho_id xd)) - |xi|^2 E_i]
for the desired layer d and the interfering layer i (ml), which is where the deliberate misreadings below can be expressed.  The
receiver's 16QAM metric is M / 2 on inputs shifted right by `shift`: 2^-shift / 2 (its y0 / sqrt 10 is Re(xd* z_d), its channel
term |xd|^2 E_d / 2).  Its QPSK metric is M / 2 as well and its output is shifted right by 4 more: 2^-shift / 32.
qpsk_interference_weight scales the bracket of a QPSK pair: 1 is max-log; the default 1 / sqrt 2 is what the reference's
QPSK-QPSK detector computes (it forms |(rho_r +- rho_i) / (2 sqrt 2) -+ y1 / 2|, sqrt 2 short of |psi| |x| with |x| = 1 / sqrt 2),
which the product reproduces bit for bit.

`mut` names ONE deliberate misreading (MUTATIONS); the tests use it to show that their cases would notice it.

BOUNDS: per (receiver, Qm) the worst deviation, in LSB of the LLR, of the numpy restatement of the reference from this model
over every RE of every case of case_list() (test_rx_float_host.py measures and prints it), and the bound = ceil(1.5 x that) to which the
restatement, the CPU forms and the GPU kernels are held."""
import numpy as np

BOUNDS = {
    # (receiver, Qm): (measured, bound)
    ("single", 2): (1.29, 2), ("single", 4): (4.85, 8), ("single", 6): (6.99, 11), ("single", 8): (7.31, 11),
    ("mmse", 6): (7.80, 12), ("mmse", 8): (7.56, 12),
    ("ml", 2): (1.86, 3), ("ml", 4): (25.40, 39),
}
MUTATIONS = {
    "single": ("first_antenna_energy",),
    "mmse": ("b_c_exchanged", "nvar_on_one_entry", "no_conjugate_in_hh"),
    "ml": ("rho_conjugated", "rho_exchanged", "int_mag_from_desired", "a_sq_dropped", "interference_abs_inverted", "mag_class_exchanged",
           "bits_1_2_exchanged"),
}
NORM = {2: 2.0, 4: 10.0, 6: 42.0, 8: 170.0}
QPSK_REFERENCE_WEIGHT = 1.0 / np.sqrt(2.0)


def _cplx(a):
    a = np.asarray(a, np.int16).astype(np.float64)
    return a[..., 0] + 1j * a[..., 1]


def bits_of(Qm):
    """uint8 [2^Qm, Qm]: bit k of candidate i is bit k of i"""
    return ((np.arange(1 << Qm)[:, None] >> np.arange(Qm)) & 1).astype(np.uint8)


def points(Qm):
    """complex128 [2^Qm]: the point of 38.211 5.1.2 .. 5.1.5 for the bits b0 .. b(Qm-1) = bits_of(Qm)[i]"""
    s = 1.0 - 2.0 * bits_of(Qm)

    def axis(ax):
        lev = np.ones(1 << Qm)
        for k in range(Qm // 2 - 1, 0, -1):                   # innermost bracket first
            lev = 2.0 ** (Qm // 2 - k) - s[:, ax + 2 * k] * lev
        return s[:, ax] * lev
    return (axis(0) + 1j * axis(1)) / np.sqrt(NORM[Qm])


def demap(v, unit, Qm):
    """float64 [n, Qm]: the nested-distance LLRs of complex v [n] with E (or K) = unit [n]"""
    lv = [np.stack([v.real, v.imag], -1)]
    for k in range(1, Qm // 2):
        lv.append((2.0 ** (Qm // 2 - k) / np.sqrt(NORM[Qm]) * unit)[:, None] - np.abs(lv[-1]))
    return np.concatenate(lv, -1)


# ---------------------------------------------------------------------------------------------------------
# single layer
# ---------------------------------------------------------------------------------------------------------
def single_layer(rx, ch, Qm, shift, mut=None):
    """float64 [nb_re, Qm]"""
    assert mut in (None,) + MUTATIONS["single"]
    r, h = _cplx(rx), _cplx(ch)
    z = (h.conj() * r).sum(0)
    E = (np.abs(h[:1] if mut == "first_antenna_energy" else h) ** 2).sum(0)
    sc = 2.0 ** -shift
    return demap(z * sc, E * sc, Qm) / (8.0 if Qm == 2 else 1.0)


# ---------------------------------------------------------------------------------------------------------
# two layers, MMSE
# ---------------------------------------------------------------------------------------------------------
def mmse(rx, ch, Qm, shift, nvar, mut=None, adjugate=False):
    """(llr float64 [nb_re, 2, Qm], xhat complex128 [nb_re, 2], K float64 [nb_re]).  xhat comes out of numpy.linalg.solve; the
    misreadings are expressed on the adjugate form adj(G) z / det(G), which `adjugate` selects without one (the tests compare)"""
    assert mut in (None,) + MUTATIONS["mmse"] and Qm in (6, 8)
    r, h = _cplx(rx), _cplx(ch)                                # [n_rx, n], [2, n_rx, n]
    nb_re = r.shape[1]
    n = (nb_re + 3) & ~3                                       # whole quads; zero channels behind nb_re
    r = np.concatenate([r, np.zeros((r.shape[0], n - nb_re))], 1)
    h = np.concatenate([h, np.zeros(h.shape[:2] + (n - nb_re,))], 2)
    sc = 2.0 ** -shift
    HhH = np.einsum("lan,man->nlm", h.conj(), h)               # [n, 2, 2]: entry (l, m) = h_l^H h_m
    G = HhH * sc + nvar * np.eye(2)
    if mut == "nvar_on_one_entry":
        G[:, 1, 1] -= nvar
    z = np.einsum("lan,an->nl", h if mut == "no_conjugate_in_hh" else h.conj(), r)
    det = (G[:, 0, 0] * G[:, 1, 1] - G[:, 0, 1] * G[:, 1, 0]).real
    if mut is None and not adjugate:
        xhat = np.zeros((n, 2), np.complex128)
        ok = det > 0
        xhat[ok] = np.linalg.solve(HhH[ok] + (nvar / sc) * np.eye(2), z[ok][..., None])[..., 0]
    else:
        B, Cc = (G[:, 1, 0], G[:, 0, 1]) if mut == "b_c_exchanged" else (G[:, 0, 1], G[:, 1, 0])
        adj_z = np.stack([G[:, 1, 1] * z[:, 0] - B * z[:, 1], G[:, 0, 0] * z[:, 1] - Cc * z[:, 0]], 1) * sc
        xhat = adj_z / np.where(det > 0, det, 1.0)[:, None]
    quad = np.floor(det / 4.0).reshape(-1, 4).sum(1)
    b = np.floor(np.log2(np.maximum(quad, 1.0))) + 1 - 8
    K = det * 2.0 ** -np.repeat(b, 4)
    llr = np.stack([demap(K * xhat[:, l], K, Qm) for l in range(2)], 1)
    return llr[:nb_re], xhat[:nb_re], K[:nb_re]


# ---------------------------------------------------------------------------------------------------------
# two layers, max-log ML
# ---------------------------------------------------------------------------------------------------------
def _llr_scale(Qm, shift):
    return 2.0 ** -shift / (32.0 if Qm == 2 else 2.0)


def _bit_llrs(best, Qm):
    """best float64 [n, 2^Qm]: the metric maximised over the other layer -> [n, Qm]"""
    bits = bits_of(Qm)
    return np.stack([best[:, bits[:, k] == 0].max(1) - best[:, bits[:, k] == 1].max(1) for k in range(Qm)], 1)


def ml_exhaustive(rx, ch, Qm, shift):
    """float64 [nb_re, 2, Qm]: max-log by definition, over all 2^(2 Qm) pairs of -|r - h0 x0 - h1 x1|^2"""
    r, h = _cplx(rx), _cplx(ch)
    x = points(Qm)
    resid = r[:, :, None, None] - h[0][:, :, None, None] * x[None, None, :, None] - h[1][:, :, None, None] * x[None, None, None, :]
    M = -(np.abs(resid) ** 2).sum(0)                            # [n, x0, x1]
    return np.stack([_bit_llrs(M.max(2), Qm), _bit_llrs(M.max(1), Qm)], 1) * _llr_scale(Qm, shift)


def ml(rx, ch, Qm, shift, qpsk_interference_weight=QPSK_REFERENCE_WEIGHT, mut=None):
    """float64 [nb_re, 2, Qm]: the expanded metric, per desired layer"""
    assert mut in (None,) + MUTATIONS["ml"] and Qm in (2, 4)
    r, h = _cplx(rx), _cplx(ch)
    x = points(Qm)
    w = qpsk_interference_weight if Qm == 2 else 1.0
    z = np.einsum("lan,an->ln", h.conj(), r)
    E = (np.abs(h) ** 2).sum(1)
    rho = np.einsum("lan,man->lmn", h.conj(), h)                # rho[l, m] = h_l^H h_m
    x_sq = np.abs(x) ** 2
    xd_sq = x_sq.copy()
    if mut == "mag_class_exchanged" and Qm == 4:                # both components inner <-> both outer
        lo, hi = np.isclose(x_sq, 0.2), np.isclose(x_sq, 1.8)
        xd_sq[lo], xd_sq[hi] = 1.8, 0.2
    out = []
    for d in range(2):
        i = d ^ 1
        rho_id = rho[d, i] if mut == "rho_exchanged" else rho[i, d]
        if mut == "rho_conjugated":
            rho_id = rho_id.conj()
        E_i = E[d] if mut == "int_mag_from_desired" else E[i]
        own = 2.0 * (x.conj()[None, :] * z[d][:, None]).real - xd_sq[None, :] * E[d][:, None]                # [n, xd]
        psi = z[i][:, None] - rho_id[:, None] * x[None, :]                                                   # [n, xd]
        other = w * 2.0 * (x.conj()[None, None, :] * psi[:, :, None]).real                                   # [n, xd, xi]
        if mut != "a_sq_dropped":
            other = other - x_sq[None, None, :] * E_i[:, None, None]
        if mut == "interference_abs_inverted" and Qm == 4:
            # xi = b0 + 2 b1 + 4 b2 + 8 b3: the best signs (b0, b1), then the worse amplitude (b2, b3) per dimension
            t = other.reshape(other.shape[:2] + (2, 2, 2, 2))                                                # [.., b3, b2, b1, b0]
            best = t.max((4, 5)).min((2, 3))
        else:
            best = other.max(2)
        L = _bit_llrs(own + best, Qm)
        if mut == "bits_1_2_exchanged" and Qm == 4:
            L = L[:, [0, 2, 1, 3]]
        out.append(L)
    return np.stack(out, 1) * _llr_scale(Qm, shift)


# ---------------------------------------------------------------------------------------------------------
# the cases: channels that couple the layers
# ---------------------------------------------------------------------------------------------------------
CORRELATIONS = (0.0, 0.5, 0.8, 0.95)
GAIN = (400.0, 480.0)
SIGMA_QUIET = 3.0
SIGMA_LOUD = {2: 220.0, 4: 110.0, 6: 48.0, 8: 24.0}     # per Qm, times sqrt(n_rx / 2): a share of the exact LLRs has the wrong sign
SINGLE_LOUD = 1.5                                       # ... and times this where layer 0 is alone on the air (no interference)
LAYER1_SCALE = 0.8                                      # the cases with unequal layers: layer 1's column times this
SEGMENTS = (6, 18, 36, 240)                             # REs per segment; the last one is the measurement symbol of the level
# seed 0 unless named here: with seed 0 one RE's matched filter of layer 1 (256QAM corner points on both layers, four antennas, c =
# 0.95) passes 32767 at the level the formula gives and the receiver's 16-bit sum wraps, which the conditions on a case exclude
SEEDS = {(8, 4, 0.95, 0): 1}


def _c16(v):
    return np.clip(np.rint(np.stack([v.real, v.imag], -1)), -32768, 32767).astype(np.int16)


def case_on(name, Qm, H16, loud, rng, c=None):
    """One case on the flat channel H16 = int16 [2, n_rx, 2] over sum(SEGMENTS) REs: random points of Qm on both layers, noise sigma
    per component.  Returns a dict: name, Qm, n_rx, c, loud, sigma, bits uint8 [n, 2, Qm], rx int16 [n_rx, n, 2] (both layers on
    the air), rx1 (layer 0 alone, for the single-layer receiver), ch int16 [2, n_rx, n, 2], max_ch."""
    n, n_rx = sum(SEGMENTS), H16.shape[1]
    hq = _cplx(H16)
    bits = rng.integers(0, 2, (n, 2, Qm)).astype(np.uint8)
    x = points(Qm)[(bits.astype(np.int64) << np.arange(Qm)).sum(-1)]                          # [n, 2]
    sigma = SIGMA_LOUD[Qm] * np.sqrt(n_rx / 2.0) if loud else SIGMA_QUIET
    noise = sigma * (rng.standard_normal((n_rx, n)) + 1j * rng.standard_normal((n_rx, n)))
    both = np.einsum("la,nl->an", hq, x)
    one = hq[0][:, None] * x[None, :, 0]
    ch = np.ascontiguousarray(np.broadcast_to(H16[:, :, None, :], (2, n_rx, n, 2)))
    return dict(name=name, Qm=Qm, n_rx=n_rx, c=c, loud=bool(loud), sigma=sigma, bits=bits, rx=_c16(both + noise),
                rx1=_c16(one + (SINGLE_LOUD if loud else 1.0) * noise), ch=ch, max_ch=int(np.abs(H16.astype(np.int32)).max()))


def coupled_case(Qm, n_rx, c, loud, scale1=1.0):
    """Layer 0's column h0 has a gain of 400 .. 480 and a phase of its own per antenna; layer 1's is c e^(j theta) h0 + sqrt(1 - c^2) o,
    o the orthogonal column of the earlier end-to-end channel (h0 turned by an angle, every other antenna's sign flipped) with its
    projection on h0 taken out and scaled back to |h0|.  That column alone is orthogonal only up to the spread of the gains, and
    with three antennas not at all ((g0^2 - g1^2 + g2^2) / |h0|^2 is about 1/3); without the projection c = 0 would not mean
    uncorrelated columns.  c is then the correlation |h0^H h1| / (|h0| |h1|) up to the rounding to int16.  scale1 scales layer 1's
    column: with equal layers nothing tells which layer's magnitude a receiver took."""
    rng = np.random.default_rng(1000003 * SEEDS.get((Qm, n_rx, c, loud), 0) + 10007 * Qm + 101 * n_rx + int(round(100 * c)) * 7 + loud)
    g, ph = rng.uniform(*GAIN, n_rx), rng.uniform(0, 2 * np.pi, n_rx)
    th, th2 = rng.uniform(0, 2 * np.pi, 2)
    h0 = g * np.exp(1j * ph)
    o = h0 * np.exp(1j * th2) * (-1.0) ** np.arange(n_rx)
    o = o - np.vdot(h0, o) / np.vdot(h0, h0) * h0
    o *= np.linalg.norm(h0) / np.linalg.norm(o)
    H16 = _c16(np.stack([h0, scale1 * (c * np.exp(1j * th) * h0 + np.sqrt(1.0 - c * c) * o)]))  # [2, n_rx, 2]
    return case_on(f"Qm{Qm}-rx{n_rx}-c{c}-{'loud' if loud else 'quiet'}" + (f"-l1x{scale1}" if scale1 != 1.0 else ""), Qm, H16, loud, rng, c)


def nvars_of(case):
    """the MMSE's nvar values of a case: 0 and 2 sigma^2"""
    return (0, int(round(2 * case["sigma"] ** 2)))


def case_list(receiver):
    """Every case of a receiver: each Qm of it at every correlation, n_rx and noise level (one layer: layer 0 of the c = 0 cases);
    for the ML receiver at 16QAM also c = 0.5 with layer 1 at LAYER1_SCALE"""
    qms, ants = {"single": ((2, 4, 6, 8), (2, 4, 3)), "mmse": ((6, 8), (2, 4)), "ml": ((2, 4), (2, 4, 3))}[receiver]
    cs = CORRELATIONS[:1] if receiver == "single" else CORRELATIONS
    out = [coupled_case(Qm, n_rx, c, loud) for Qm in qms for n_rx in ants for c in cs for loud in (0, 1)]
    if receiver == "ml":
        out += [coupled_case(4, n_rx, 0.5, 0, LAYER1_SCALE) for n_rx in ants]
    return out


def segments_of(case):
    """(offset, nb_re) of the case's segments"""
    at, out = 0, []
    for nb in SEGMENTS:
        out.append((at, nb))
        at += nb
    return out
