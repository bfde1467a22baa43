"""The UL receive chain on frequency-selective channels with every DMRS port on the air, on the CPU forms (no GPU): the slots of
ul_slot_np.py through pusch_chest_segments / pusch_grid_segments, pusch_chest_host per (descriptor, antenna), ulsch_level_host and
ulsch_compensate_host (one layer) or ulsch_level_mmse_host and ulsch_mmse_2layers_host (two layers), demap_np, unscramble and the
oracle's decoder.  Unlike the bit-exact tests this one does not rest on a restatement alone: the estimates must be near a float64
channel the estimator never saw, the block must decode, and estimates one PRB or one 4-RE group off, a delay of the wrong sign or
antenna, swapped layer planes or a wrong w_f must not.

The bounds on |est - h| per component (bounds() below), term by term.  x = 2 pi max|tau| / N is the main tap's phase step per RE, G
the largest |g|, E the largest |e|, sigma the noise per component.

  noise, six sigma.  A pilot times a received value at shift 16 carries 23170 sqrt 2 / 2^16 = sigma / 2 per component, at shift 15
      sigma.  TYPE1_INTERP: a pair is two shift-16 products added, sigma / sqrt 2; an interior group takes four pairs with weight 1/4
      each: 0.354 sigma; of the first and last two groups the last is the worst, pair weights 5/8, 1/4, 1/8: 0.484 sigma.
      TYPE2_INTERP: the mean of two shift-15 products, 0.707 sigma.  TYPE1_AVG: the mean of six, 0.408 sigma.  TYPE2_AVG: of four, 0.5.
  table.  An entry is rounded to 1 / 256: a rotation moves a component by at most (|re| + |im|) / 512 <= sqrt 2 |h| / 512; TYPE1_INTERP
      rotates twice, TYPE2_INTERP once, the averaging modes not at all.
  truncations, worst case.  TYPE1_INTERP: two floors in the pair (2), through the rotation (x sqrt 2, + 1 for its floor), up to eight
      filter terms rounded to a unit each (8), through the second rotation (x sqrt 2, + 1): 18.  TYPE2_INTERP: two floors, the halving,
      the & ~3 (3), one rotation: 10.  Averaging: the products' floors average to 1, the division adds 1: 3 generously.
  second tap.  Every estimate is a combination of pilot-RE channels with unit-modulus factors and weights that add up to one, so the
      second tap contributes at most E to it, and E to the true channel: 2 E whatever tau2 is.
  main tap, interpolating modes.  TYPE1_INTERP gives both pilots of a pair the pair's mean, which belongs half-way between them:
      after the forward rotation one carries G e^(-ix) cos x and the other G e^(+ix) cos x.  An interior group weighs four of each
      with 1/8: the sines cancel and G (1 - cos x) stays.  The one-sided filters of the first and last two groups do not cancel
      them: the signed weights add up to 1/4, 1/4, 1/4 and (last group) 1/2, so G sin(x) / 2 more.  A port with delta = 1 is
      rotated by the table entry of the RE before its pilot: the estimates sit one RE off, G 2 sin(x / 2) more everywhere.
      TYPE2_INTERP takes the mean of two adjacent pilots for the first of them and rotates on from there: G sin(x / 2).
  main tap, averaging modes: the spread of h over one PRB.  |e^(ia) - e^(ib)| <= |a - b|, so the mean of the pilots differs from
      h(k) by at most G x times the mean distance of k from the pilots: 6 for TYPE1_AVG (k = 11, pilots at 0, 2 .. 10) and 7.5 for
      TYPE2_AVG (k = 11, pilots at 0, 1, 6, 7).  Every RE of a PRB is alike here: one bound for interior and edge.
  the other port (two layers).  Ports 0 and 1 share the comb and differ in the sign of every other pilot, so the other port's
      channel enters a pilot pair as half the difference of its two values: the change of h within one pilot pair.  Type 1 pairs
      are two REs apart, |1 - e^(-2ix)| / 2 = sin x; type 2 pairs one RE apart, sin(x / 2); times G, plus at most E for the second tap.
      The delay compensation does not remove it and the filters do not average it out: it has the same sign in every pair.

Measured on these slots, restatement error / bound (interior, edge), are in DESIGN section 4.12; the conditions below hold them to
at least 1.5 x headroom and the bound to less than a quarter of the smallest |g|.

The perturbations.  A perturbed estimate must miss the bound of the interior REs or that of the edge REs by three times -- the two
checks a wrong kernel would have to pass.  The rolls are circular over the allocation, as a kernel that wrote one group late would
leave the first group with whatever lay there.  The averaging modes take no delay (ul_slot_np.py): there the two delay perturbations
must change nothing at all, and that is what is asserted.  For the port with delta = 1 the one-RE offset the reference builds in
keeps the delay at 2, too little for a wrong sign to show above the noise of one layer: its case checks the rolls alone.

TYPE1_INTERP with two ports is the one case that cannot have a wrong delay three times above the bound.  With u = G x: the other
port's leak puts u into the bound, the edge groups another u / 2, and the terms that do not depend on the delay add about 37.  A
negated delay leaves a slope of 2 x that the filter reads 2.5 REs (interior) or 3.5 REs (last group) from its centre: an error of
at most 5 u or 7 u, about 0.93 of that per component.  Three times the bound asks 4.65 u >= 3 (u + 34) in the interior, u >= 62,
or 6.5 u >= 3 (1.5 u + 37) at the edge, u >= 56; but 1.5 x headroom over the restatement's interior error, which is the leak
itself (u + 6 measured), asks u + 34 >= 1.5 (u + 6), u <= 50, and a bound below G / 4 = 118 asks 1.5 u + 37 < 118, u < 54.  The
case keeps the two conditions on the bound (u = 38) and holds a wrong delay to twice the bound (delay_factor) and to a block
that no longer decodes; every other perturbation of it, and every perturbation of every other case, is held to three times."""
import numpy as np
import pytest

import ul_slot_np as U

NAMES = [c["name"] for c in U.CASES]
NOISE_W = {U.T1I: (0.354, 0.484), U.T2I: (0.707, 0.707), U.T1A: (0.408, 0.408), U.T2A: (0.5, 0.5)}
TRUNC = {U.T1I: 18.0, U.T2I: 10.0, U.T1A: 3.0, U.T2A: 3.0}
ROTATIONS = {U.T1I: 2, U.T2I: 1, U.T1A: 0, U.T2A: 0}


def bounds(sl):
    """(interior, edge) bound on |est - h| per component, from the model alone: see the module docstring"""
    c = sl["case"]
    mode, G, E = c["mode"], float(np.abs(sl["g"]).max()), float(np.abs(sl["e"]).max())
    x = 2 * np.pi * max(abs(t) for t in c["tau"]) / c["N"]
    common = ROTATIONS[mode] * np.sqrt(2.0) * (G + E) / 512 + TRUNC[mode] + 2 * E
    if c["n_layers"] == 2:
        common += G * (np.sin(x / 2) if mode & 1 else np.sin(x)) + E
    if mode == U.T1I:
        main = G * (1 - np.cos(x)) + (G * 2 * np.sin(x / 2) if c["ports"][0] & 2 else 0.0)
        main = (main, main + G * np.sin(x) / 2)
    elif mode == U.T2I:
        main = (G * np.sin(x / 2),) * 2
    else:
        main = (G * x * (6.0 if mode == U.T1A else 7.5),) * 2
    return tuple(6 * c["sigma"] * NOISE_W[mode][i] + common + main[i] for i in range(2))


def perturbations(m, sl):
    """name -> (perturbed ul_ch, whether the block must fail with it); None in place of ul_ch: the mode takes no delay"""
    c = sl["case"]
    ch = U.estimate_host(m, sl)
    P = U.planes_of(sl, ch)
    out = {}
    for name, shift in (("rolled by one PRB", 12), ("rolled by one 4-RE group", 4)):
        out[name] = (ch.copy(), True)
        U.planes_of(sl, out[name][0])[:] = np.roll(P, shift, axis=2)
    if c["delay_checks"]:
        takes_delay = c["mode"] in (U.T1I, U.T2I)
        out["est_delay negated"] = (U.estimate_host(m, sl, delay=-sl["delay"]), True)
        if c["n_rx"] > 1:
            d = sl["delay"].reshape(-1, c["n_rx"]).copy()
            d[:, [0, 1]] = d[:, [1, 0]]
            out["est_delay of antennas 0 and 1 swapped"] = (U.estimate_host(m, sl, delay=d.reshape(-1)), False)
        if not takes_delay:
            for k in [k for k in out if k.startswith("est_delay")]:
                assert np.array_equal(out[k][0], ch), (c["name"], k, "an averaging mode read est_delay")
                out[k] = (None, False)
    if c["n_layers"] == 2:
        out["layer planes swapped"] = (ch.copy(), True)
        U.planes_of(sl, out["layer planes swapped"][0])[:] = P[::-1]
        wrong = [sl["csegs"][0], dict(sl["csegs"][1], port=sl["csegs"][0]["port"])]
        out["layer 1 estimated with port 0's w_f"] = (U.estimate_host(m, sl, csegs=wrong), False)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_selective_slot_on_the_cpu_forms(built, name):
    import openairinterface5g_amd as pkg
    m = pkg.ldpc
    sl = U.slot_of(m, name)
    c = sl["case"]
    # the descriptors: the second layer's set lies n_rx ch_stride behind the first and its delays behind the first's
    assert [s["port"] for s in sl["csegs"]] == list(c["ports"])
    assert [s["ch_off"] - sl["csegs"][0]["ch_off"] for s in sl["csegs"]] == [l * c["n_rx"] * sl["ch_stride"] for l in range(c["n_layers"])]
    assert [s["delay_off"] for s in sl["csegs"]] == [l * c["n_rx"] for l in range(c["n_layers"])]
    assert all(g["ch_off"] == sl["csegs"][0]["ch_off"] for g in sl["gsegs"] + sl["first"])
    if c["n_layers"] == 2:
        assert {g["pattern"] for g in sl["gsegs"]} == {U.FULL, U.DMRS2 if c["mode"] & 1 else U.DMRS1}
    # 1. the host form against the literal restatement of the reference, on this slot
    ch = U.estimate_host(m, sl)
    ref = U.estimate_ref(sl)
    assert np.array_equal(ch, ref), (name, np.argwhere(ch != ref)[:4])
    written = ch != U.FILL
    assert written.reshape(c["n_layers"] * c["n_rx"], -1).sum(1).tolist() == [2 * 12 * c["rb"]] * (c["n_layers"] * c["n_rx"])
    # 2. near the true channel: bounds from the model, conditions on the case
    b_int, b_edge = bounds(sl)
    e_int, e_edge = U.est_error(sl, ref)
    print(f"{name}: restatement error {e_int:.0f} / bound {b_int:.0f} interior, {e_edge:.0f} / {b_edge:.0f} edge; "
          f"|g| {np.abs(sl['g']).min():.0f} .. {np.abs(sl['g']).max():.0f}")
    assert b_edge < np.abs(sl["g"]).min() / 4, (name, b_edge, "the channel is too hard for this mode")
    assert 1.5 * e_int <= b_int and 1.5 * e_edge <= b_edge, (name, e_int, b_int, e_edge, b_edge)
    # 3. the block decodes
    lv, rec = U.front_records(sl, ch, m)
    lv_np, rec_np = U.front_records(sl, ch, None)
    assert lv == lv_np and np.array_equal(rec, rec_np), "the CPU forms against the numpy receivers"
    got, ack, iters = U.decode_record(sl, rec)
    assert ack and np.array_equal(got, sl["pay"]), (name, iters)
    assert max(iters) <= U.MAX_ITER
    # 4. a subtly wrong estimator would be noticed
    for what, (chp, must_fail) in perturbations(m, sl).items():
        if chp is None:
            continue
        p_int, p_edge = U.est_error(sl, chp)
        print(f"    {what}: error {p_int:.0f} interior ({p_int / b_int:.1f} x bound), {p_edge:.0f} edge ({p_edge / b_edge:.1f} x)")
        f = c["delay_factor"] if what.startswith("est_delay") else 3.0
        assert p_int >= f * b_int or p_edge >= f * b_edge, (name, what, p_int, b_int, p_edge, b_edge)
        if what in c["survives"]:                         # QPSK: the estimate misses its bound, the block decodes all the same
            got, ack, iters = U.decode_record(sl, U.front_records(sl, chp, m)[1])
            assert must_fail and ack and np.array_equal(got, sl["pay"]), (name, what, iters)
        elif must_fail:
            got, ack, iters = U.decode_record(sl, U.front_records(sl, chp, m)[1])
            assert not ack and max(iters) > U.MAX_ITER and not np.array_equal(got, sl["pay"]), (name, what, iters)
