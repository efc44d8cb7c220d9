"""GPU: the extraction's variance and optimal kernels at the sizes they are written for (wayne_amd/csrc/k_extract.h): S up
to 1024 (kExtractMaxS), 15 read intervals (kExtractProducts = 17), 256 channels (kChanMaxChannels), a column hull of 384
(kChanMaxHull).  The siblings (test_variance_gpu, test_optimal_gpu, test_fixed_profile_gpu) stop at S = 266, R = 4, 23
channels and a hull of 220; here the same numpy laws (variance_law, optimal_law, fixed_profile_law, channel_law, crrej_law,
extraction_law, spectra_layout_law) are applied to the reads of the SAME slot with the laws' own tolerances -- no new law,
no new bound.  Every element the device delivers is compared.

Frames.  tiny512 (S = 522: a second trip of every `x += 512` loop, a ninth column tile of 10 columns, room for a 384-column
hull) with the star 10 times brighter (3e6 electrons, as small256) and x_ref moved through frame_kwargs' override: the
visit's own x_ref = 330 leaves everything right of column 276 dark.  The channel plans (A) take x_ref = 580, the first
order on columns 372 .. 508 and its red wing up to the frame's border (500 for the plan against the left edge, the
visit's own for the narrow plan beyond it).  The wide frames (B) take x_ref = 560: the order on columns 352 .. 488, its
red wing fading out near column 505, so that at H = 1, 8 and 16 alike ok(x) takes both values among the columns 496 ..
521 (by the law on CPU-oracle reads: true up to about column 505, 511 and 519) and is true beyond column 511 at H = 16; at 580
every one of those columns is ok at H = 8 and 16.  Columns 512 .. 516 then hold the sky's photons, not the star's, above
their window's read noise; the star's reach them in A's plans and in D.  ramp16_128 (S = 138, 15 read intervals, the
star 30 times brighter as tiny128's in the siblings).  cfg2 (S = 1014 + 10, 15 intervals).

Path -> covering case (A: test_channels_at_both_caps*, B: test_frames_wider_than_one_stride, C: test_fifteen_read_intervals,
D: test_everything_at_once_on_the_full_array)

    k_extract_bins<T, CR, true>: strips 4, 5 of vr[] (hull > 256), passes k >= 1 of the P / Q / V gathers,    A (every plan;
      redv ending with buf at C = 256, the write-out loops beyond i = 64 k                                     CR, f64, u16:
                                                                                                               the first), D
    k_extract_bins_finish<true>: threads b >= 64                                                              A, D
    k_extract_bins_opt<T, CR, FIXED>, both FIXED: tid >= 256 forming shW / shS0, bd[wave][c] up to c = 415    A (left / right
      with the halo outside the frame on either side, passes kk >= 1, red at 3 C = 768, write-out beyond 512   edge: the halo
                                                                                                               outside), D
    k_extract_bins_opt_finish: threads b >= 64                                                                A, D
    k_extract_finish<CR, true>: the second trip of the column loops -- shV[x], spectra_var, with CR shN        B, D
    k_extract_optimal_finish: the second trip; the S0 / SV0 window across x = 511 / 512 and at x = S - 1       B (S = 522), D
                                                                                                               (S = 1024)
    k_extract_optimal, k_extract_profile, k_extract_optimal_fixed: more than 5 column tiles, a last tile of    B (10 columns),
      10 columns, a last tile that is full and ends with the frame                                             D (full)
    extract_term<T, CR>: products 5 .. 15, first_chunk searched over 15 products, row_off[p] up to p = 15,     C (planes of
      mask bits 8 .. 14 in the last-read correction                                                            all 16
                                                                                                               windows), D

Mutants (scripts/mutation_audit.py, caps_*; each drops or replaces a term, none moves an index or a bound).  Each was run
once against this module and once against the rest of the GPU tests that ask for an extraction (test_variance_gpu,
test_optimal_gpu, test_fixed_profile_gpu, test_channels_gpu, test_crrej_gpu, test_extraction_gpu, test_expected_gpu,
test_device_fits_gpu, test_visit_science_gpu: 367 tests; no other GPU test launches a kernel of k_extract.h), and so was
caps_all, the seven edits in one library.  The rest let every one of them through, 367 passed each time.  Killed here by
(A1: the three 1.5-pixel plans of test_channels_at_both_caps with both window sets, and its f64 / u16 / crrej cases; A2:
the four narrow cases; B, C, D as above):

    caps_bins_var_strips    vr[s] = 0 for the strips s >= 4                  A1, D      (channels_var off by up to 0.96)
    caps_bins_var_passes    no V[k] gather for k >= 1                        A1, A2, D  (channels_var)
    caps_binsopt_ok_256     shW = 0 for tid >= 256                           A1, D      (channels_opt)
    caps_binsopt_halo       d = 0 in bd's columns >= 384 (own profile)       A1, D      (channels_opt)
    caps_finish_skyvar_512  no B^2 sky_var in spectra_var for x >= 512       A1, A2, B, D  (spectra_var)
    caps_optimal_ok_512     ok false for x >= 512 in the finish kernel       B, D, and A's plans with light beyond column 511
                                                                             (over the order, both at the right edge)
    caps_term_flag_bit      interval p's flag from bit min(p, 7)             C, D       (channels_var and the optimal sums)

Every other case of the module passed on each mutant.

Measured on the device, the worst deviation from the law per product over the whole module, in the unit of its bound
(allowed: 1e-9; optimal 2e-9; optimal_var and channels_opt_var 4e-9; the profile planes equal the law to the bit):
spectra / M 1.9e-15, sky / M_sky 2.4e-16, spectra_var 1.8e-15, sky_var 8.3e-16, channels / M 9.5e-16, channels_var
7.3e-16, optimal W / M_U 3.3e-15, optimal_var 2.4e-15, channels_opt / M 2.6e-15, channels_opt_var 4.2e-15.  No exposure
had an undecided flag: exposure 0 of each visit, the first tried, is the one used.  The module takes 12 s, 6.7 s of them
the cfg2 case, of which 6.5 s are the numpy laws on the 1024 frame.
"""
import time

import numpy as np
import pytest

import channel_law
import crrej_law
import extraction_law as law
import fixed_profile_law as fpl
import optimal_law
import spectra_layout_law as sll
import test_fixed_profile_gpu as tfp
import variance_law
from wayne_amd import extraction

pytestmark = pytest.mark.gpu

RN = tfp.RN
BRIGHT = {"tiny512": 10.0, "ramp16_128": 30.0, "cfg2": 1.0}
X_REF = 580.0                    # tiny512: the first order on columns 372 .. 508 (see above)
X_REF_B = 560.0                  # ... and on 352 .. 488, its red wing fading out before the frame ends (case B)
A_UM, PX_UM = 1.0, 2.0 ** -10    # the hand-made solution lambda = 1 + 2^-10 u: (e - a) / b is exact for edges on quarter pixels
WORST = {}                       # product -> the worst deviation seen, in the unit of its law's bound


def note(product, value):
    WORST[product] = max(WORST.get(product, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    print("caps: worst deviations over the module: " + ", ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


def over_of(v, x_ref=None, crrej=False, rate=30.0):
    over = dict(stellar_flux=np.asarray(v.stellar_flux) * BRIGHT[v.name])
    if x_ref is not None:
        over["x_ref"] = x_ref
    if crrej:
        over["cosmic_rate"] = tfp.busy_rate(v, rate)
    return over


def rel(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return float((np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).max()) if want.size else 0.0


class Checked(object):
    """What one run of a slot delivered and what the laws make of the same reads."""


def check(ctx, slot, v, plan, reads, what, box=True):
    """Every product the slot's plan asks for against its law, on `reads`.  box=False: the box products (spectra, sky,
    counts, channels and their variances), which the optimal options do not touch, were checked on an earlier run."""
    pl = tfp.planes_of(v)
    R, S = v.NSAMP - 1, pl.S
    cr = tfp.crrej_of(plan)
    c = Checked()
    c.plan = plan
    c.spectra, c.sky = ctx.download_spectra(slot)
    c.spectra_var, c.sky_var, c.channels_var = ctx.variances(slot)
    assert c.spectra.shape == c.spectra_var.shape == (R + 1, S) and c.sky.shape == c.sky_var.shape == (R + 1,), what
    ch = plan.channels
    chan = {}
    if ch is not None:
        chan = dict(edges=ch.edges_um, wl_a=plan.row_solution[0], wl_b=plan.row_solution[1], flat=tfp.flat_of(v) if ch.flat else None)
        c.channels = ctx.channels(slot)
        assert c.channels.shape == c.channels_var.shape == (R + 1, ch.n), what
    if box:
        if cr is not None:
            want = crrej_law.restate(reads, pl, plan.row_windows, plan.bg_cols, plan.steps, cr[0], cr[1])
            assert not want.undecided.any(), "%s: %d undecided pixels -- take another exposure" % (what, want.undecided.sum())
            c.mask, c.rejected = ctx.download_crmask(slot), ctx.rejected(slot)
            np.testing.assert_array_equal(c.mask, want.mask, err_msg=what)
            np.testing.assert_array_equal(c.rejected, want.n_rejected, err_msg=what)
            crrej_law.assert_parity(c.spectra, c.sky, want, what)
            M, M_sky, spectra, sky = want.M, want.M_sky, want.spectra, want.sky
        else:
            spectra, sky, M, M_sky = law.restate(reads, pl, plan.row_windows, plan.bg_cols, plan.steps)
            law.assert_parity(c.spectra, c.sky, reads, pl, plan.row_windows, plan.bg_cols, plan.steps, what)
        note("spectra / M", (np.abs(c.spectra - spectra) / np.maximum(M, 1e-300)).max())
        note("sky / M_sky", (np.abs(c.sky - sky) / np.maximum(M_sky, 1e-300)).max())
        c.want_var = variance_law.restate(reads, pl, plan.row_windows, plan.bg_cols, plan.variance.read_noise, plan.steps, cr, **chan)
        variance_law.assert_parity(c.spectra_var, c.sky_var, c.channels_var, c.want_var, what)
        note("spectra_var", rel(c.spectra_var, c.want_var.spectra_var))
        note("sky_var", rel(c.sky_var, c.want_var.sky_var))
        if ch is not None:
            note("channels_var", rel(c.channels_var, c.want_var.channels_var))
            c.want_channels = channel_law.restate(reads, pl, plan.row_windows, plan.bg_cols, ch.edges_um, plan.row_solution[0],
                                                  plan.row_solution[1], plan.steps, chan["flat"], cr, sky=c.sky)
            channel_law.assert_parity(c.channels, c.want_channels, what)
            note("channels / M", (np.abs(c.channels - c.want_channels.channels) / np.maximum(c.want_channels.M, 1e-300)).max())
    opt = plan.optimal
    if opt is None:
        return c
    H, prof = opt.half_width, None if opt.profile is None else opt.profile.planes
    c.optimal, c.optimal_var = ctx.optimal(slot)
    box_arrays = (c.spectra, c.sky, c.spectra_var, c.sky_var)
    if prof is None:
        c.want_optimal = optimal_law.restate(reads, pl, plan.row_windows, H, plan.variance.read_noise, *box_arrays, plan.steps, cr)
    else:
        c.want_optimal = fpl.restate(reads, pl, plan.row_windows, H, plan.variance.read_noise, prof, *box_arrays, plan.steps, cr)
    w = c.want_optimal
    optimal_law.assert_parity(c.optimal, c.optimal_var, w, c.spectra, c.spectra_var, what)
    if w.ok.any():
        note("optimal W / M_U", (np.abs(c.optimal - w.optimal)[w.ok] * w.W[w.ok] / np.maximum(w.M_U[w.ok], 1e-300)).max())
        note("optimal_var", rel(c.optimal_var[w.ok], w.optimal_var[w.ok]))
    if opt.deliver_profile:
        c.planes = ctx.profile_planes(slot)
        want = fpl.planes(reads, pl, plan.row_windows, H, c.sky, plan.steps, cr)
        assert c.planes.shape == want.shape == (sum(fpl.heights(plan.row_windows)), S), what
        assert c.planes.tobytes() == want.tobytes(), "%s: planes differ by up to %g" % (what, np.abs(c.planes - want).max())
    if opt.channels:
        c.channels_opt, c.channels_opt_var = ctx.optimal_channels(slot)
        c.want_optch = fpl.channels(reads, pl, plan.row_windows, H, plan.variance.read_noise, prof, *box_arrays, ch.edges_um,
                                    plan.row_solution[0], plan.row_solution[1], plan.steps, chan["flat"], cr)
        fpl.assert_channel_parity(c.channels_opt, c.channels_opt_var, c.want_optch, what)
        note("channels_opt / M", (np.abs(c.channels_opt - c.want_optch.channels_opt) / np.maximum(c.want_optch.M, 1e-300)).max())
        note("channels_opt_var", rel(c.channels_opt_var, c.want_optch.channels_opt_var))
    return c


def run_plan(ctx, slot, plan):
    ctx.set_extraction(slot, plan)
    ctx.run(slot)


def sigmas(flux, var):
    with np.errstate(all="ignore"):
        return np.where(var > 0.0, flux / np.sqrt(var), 0.0)


def assert_the_far_channels_are_lit(c, what):
    """Light where only the cap cases look: a channel of index >= 192 and -- where the hull has them -- a column 320 or more
    into the hull stand 3 sigma above their noise (so their law's magnitude M, which is at least |flux|, stands above
    the read-noise floor), by the LAW's values."""
    u_lo, u_hi = c.plan.hull
    assert np.abs(c.want_channels.channels).max() > 1000.0, what
    assert (sigmas(c.want_channels.channels, c.want_var.channels_var)[:, 192:] > 3.0).any(), what
    if u_hi - u_lo > 320:
        assert (sigmas(c.spectra, c.spectra_var)[:, u_lo + 320:u_hi] > 3.0).any(), what


def assert_the_far_optimal_channels_are_lit(c, what):
    u_lo, u_hi = c.plan.hull
    ok = c.want_optch.ok[:, u_lo:u_hi]
    assert ok.any() and (~ok).any(), what                            # both branches of e, k and ev inside the hull
    assert (sigmas(c.want_optch.channels_opt, c.want_optch.channels_opt_var)[:, 192:] > 3.0).any(), what
    assert (c.want_optch.M[:, 192:] > 1000.0).any(), what
    if u_hi - u_lo == extraction.MAX_HULL:
        # the optimal branch is taken beyond thread 256 and, with the widest profile, next to the right halo
        assert ok[:, 256:].any() and ok[:, 320:].any(), what
        if c.plan.optimal.half_width == 16:
            assert ok[:, 368:].any(), what


# ---- A: 256 channels and a hull of 384 columns at once, on tiny512 ----

S512 = 522
# name -> (x_ref or None for the visit's own, first edge in columns, channel width in columns, the hull)
A_PLANS = {
    "over the first order": (X_REF, 130.0, 1.5, (130, 514)),
    "against the left edge": (500.0, 0.0, 1.5, (0, 384)),                  # (the order on 292 .. 428: light up to the hull's end)
    "against the right edge": (X_REF, float(S512 - 384), 1.5, (S512 - 384, S512)),
    "narrow, beyond the left edge": (None, -6.0, 0.75, (0, 186)),         # channels 0 .. 7 wholly outside the frame
    "narrow, beyond the right edge": (X_REF, 336.0, 0.75, (336, S512)),   # channels 248 .. 255 wholly outside the frame
}
# a one-row window, one shorter than the 8 waves, one of 11 chunks and 5 rows that ends with the frame's interior
HAND_WINDOWS = [(180, 181), (184, 189), (160, S512 - 5)]


def hand_channels(u0, width, n=256):
    edges = A_UM + PX_UM * (u0 + width * np.arange(n + 1))
    assert ((edges - A_UM) / PX_UM == u0 + width * np.arange(n + 1)).all()
    return extraction.Channels(edges), (np.full(S512, A_UM), np.full(S512, PX_UM))


def caps_case(name, hand, out_dtype=np.float32, crrej=False):
    """One upload; five runs: the flat on with the exposure's own and a made-up profile at H = 1 and 16, then the flat off."""
    v = tfp.visit("tiny512")
    ctx = tfp.engine_of(v).ctx
    x_ref, u0, width, hull = A_PLANS[name]
    over = over_of(v, x_ref, crrej)
    ch, sol = hand_channels(u0, width)
    windows = HAND_WINDOWS if hand else tfp.descriptor(v, 0, extraction.ExtractionOptions(), out_dtype, **over)[1].extraction_plan.row_windows
    prof = extraction.Profile(tfp.made_up_profile(windows, S512), fpl.heights(windows))

    def plan_of(flat, H, supplied):
        return extraction.Extraction(windows, crrej=crrej or None, channels=ch.with_flat(flat), row_solution=sol,
                                     variance=extraction.Variances(RN),
                                     optimal=extraction.Optimal(H, profile=prof if supplied else None, channels=True))

    first = plan_of(True, 1, False)
    assert first.hull == hull and ch.n == extraction.MAX_CHANNELS == 256
    if width == 1.5:
        assert hull[1] - hull[0] == extraction.MAX_HULL == 384
    desc, _ = tfp.descriptor(v, 0, first, out_dtype, **over)
    ctx.upload(0, desc)
    ctx.run(0)
    reads = ctx.download(0)
    what = "%s, %s windows, %s, crrej %d" % (name, "hand-made" if hand else "planned", np.dtype(out_dtype).name, crrej)
    done = []
    for n, (flat, H, supplied) in enumerate([(True, 1, False), (True, 1, True), (True, 16, False), (True, 16, True), (False, 16, True)]):
        plan = plan_of(flat, H, supplied)
        if n:
            run_plan(ctx, 0, plan)
        label = "%s: flat %d H %d %s profile" % (what, flat, H, "supplied" if supplied else "own")
        c = check(ctx, 0, v, plan, reads, label, box=n in (0, 4))
        if n in (0, 4):
            assert_the_far_channels_are_lit(c, label)
            if crrej:
                assert c.rejected.sum() > 0, label
        assert_the_far_optimal_channels_are_lit(c, label)
        done.append(c)
    assert done[0].channels.tobytes() == done[3].channels.tobytes() != done[4].channels.tobytes()      # the flat matters, H does not
    assert done[0].channels_opt.tobytes() != done[2].channels_opt.tobytes()                            # ... to the box channels
    if name.startswith("narrow"):
        outside = slice(0, 8) if "left" in name else slice(248, 256)
        for c in done:
            assert not c.channels[:, outside].any() and not c.channels_opt[:, outside].any() and not c.channels_opt_var[:, outside].any()
    if hand:
        assert fpl.heights(windows) == (1, 5, 357) and 357 % 32 == 5 and windows[2][1] == S512 - 5


@pytest.mark.parametrize("hand", [False, True], ids=["planned", "hand-made"])
@pytest.mark.parametrize("name", list(A_PLANS), ids=[n.replace(" ", "-").replace(",", "") for n in A_PLANS])
def test_channels_at_both_caps(name, hand):
    caps_case(name, hand)


@pytest.mark.parametrize("out_dtype,crrej", [(np.float64, False), (np.uint16, False), (np.float32, True)], ids=["f64", "u16", "crrej"])
def test_channels_at_both_caps_other_reads_and_rejection(out_dtype, crrej):
    caps_case("over the first order", False, out_dtype, crrej)


# ---- B: frames wider than one stride of the finish kernels, on tiny512 with its default plan ----

@pytest.mark.parametrize("crrej", [False, True], ids=["plain", "crrej"])
@pytest.mark.parametrize("out_dtype", [np.float32, np.float64, np.uint16], ids=["f32", "f64", "u16"])
def test_frames_wider_than_one_stride(out_dtype, crrej):
    v = tfp.visit("tiny512")
    ctx = tfp.engine_of(v).ctx
    pl = tfp.planes_of(v)
    S, R = pl.S, v.NSAMP - 1
    assert S == S512 and S > 512 and S % 64 == 10
    over = over_of(v, X_REF_B, crrej)
    ch = extraction.Channels.linear(*tfp.WIDE["G141"], 20)
    opts = extraction.ExtractionOptions(crrej=crrej or None, channels=ch, variance=extraction.Variances(RN), optimal=extraction.Optimal(1))
    desc, gen = tfp.descriptor(v, 0, opts, out_dtype, **over)
    base = gen.extraction_plan
    prof = extraction.Profile(tfp.made_up_profile(base.row_windows, S), fpl.heights(base.row_windows))
    ctx.upload(0, desc)
    ctx.run(0)
    reads = ctx.download(0)
    what = "tiny512 x_ref %g %s crrej %d" % (X_REF_B, np.dtype(out_dtype).name, crrej)
    n, beyond = 0, {False: False, True: False}
    for H in (1, 8, 16):
        for supplied in (None, prof):
            plan = base.with_optimal(extraction.Optimal(H, profile=supplied))
            if n:
                run_plan(ctx, 0, plan)
            label = "%s H %d %s profile" % (what, H, "own" if supplied is None else "supplied")
            c = check(ctx, 0, v, plan, reads, label, box=n == 0)
            ok = c.want_optimal.ok
            assert ok[:, 496:].any() and (~ok[:, 496:]).any() and (~ok[:R]).any(), label      # both branches among the columns 496 .. 521
            beyond[supplied is not None] |= bool(ok[:, 512:].any())
            if n == 0:
                if crrej:
                    assert c.rejected.sum() > 0, label
                # every column of the second trip holds photons on top of its window's read noise, and the sky level's share
                floor = np.array([RN * RN * ((pl.gain[lo:hi] / 2.35) ** 2).sum(axis=0) for lo, hi in base.row_windows])
                assert (c.want_var.VA[:, 512:] > floor[:, 512:]).all(), label
                assert (c.want_var.B[:, 512:] > 0.0).any() and (c.want_var.sky_var > 0.0).all(), label
                assert (c.want_var.spectra_var[:, 512:] > c.want_var.VA[:, 512:]).any(), label
            n += 1
    assert beyond[False] and beyond[True], what                      # the optimal branch is taken beyond the first stride


# ---- C: fifteen read intervals, on ramp16_128 ----

@pytest.mark.parametrize("out_dtype", [np.float32, np.uint16], ids=["f32", "u16"])
def test_fifteen_read_intervals(out_dtype):
    """Exposure 0 of ramp16_128 (the first tried: no undecided flag) at 30 hits per read interval."""
    v = tfp.visit("ramp16_128")
    ctx = tfp.engine_of(v).ctx
    pl = tfp.planes_of(v)
    S, R = pl.S, v.NSAMP - 1
    assert (S, R) == (138, 15)
    over = over_of(v, None, True)
    ch = extraction.Channels.linear(*tfp.WIDE["G141"], 20)
    opts = extraction.ExtractionOptions(crrej=True, channels=ch, variance=extraction.Variances(RN),
                                        optimal=extraction.Optimal(1, deliver_profile=True, channels=True))
    desc, gen = tfp.descriptor(v, 0, opts, out_dtype, **over)
    base = gen.extraction_plan
    rows = fpl.heights(base.row_windows)
    assert len(set(map(tuple, base.row_windows))) == R + 1                     # every product has a window of its own
    assert base.row_windows[R - 1, 0] - base.row_windows[0, 0] >= 40           # the trace crosses more than 40 rows
    assert rows[R] > 2 * 32 and rows[R] % 32 != 0 and min(rows[:R]) > 32        # several chunks and a remainder
    prof = extraction.Profile(tfp.made_up_profile(base.row_windows, S), rows)
    ctx.upload(0, desc)
    ctx.run(0)
    reads = ctx.download(0)
    what = "ramp16_128 %s" % np.dtype(out_dtype).name
    n = 0
    for H in (1, 8, 16):
        for supplied in (None, prof):
            plan = base.with_optimal(extraction.Optimal(H, profile=supplied, deliver_profile=True, channels=True))
            if n:
                run_plan(ctx, 0, plan)
            label = "%s H %d %s profile" % (what, H, "own" if supplied is None else "supplied")
            c = check(ctx, 0, v, plan, reads, label, box=n == 0)
            assert c.planes.shape[0] == sum(rows) and all(c.planes[sum(rows[:p]):sum(rows[:p + 1])].any() for p in range(R + 1)), label
            ok = c.want_optimal.ok
            assert ok[5:R].any() and ok[R].any() and (~ok[:R]).any(), label
            assert c.want_optch.ok.any() and (~c.want_optch.ok).any(), label
            if n == 0:
                assert c.rejected[5:R].sum() > 0 and c.rejected[8:R].sum() > 0, label       # flags in the products 8 .. 14 ...
                assert int(c.mask.max()) >> 8 > 0, label                                    # ... on the mask's high byte
                last = c.mask[base.row_windows[R, 0]:base.row_windows[R, 1]]
                assert ((last >> 8) != 0).any(), label                                      # ... inside the last-read window
                assert np.abs(c.want_channels.channels).max() > 1000.0, label
            n += 1


# ---- D: everything at once on the 1024 array with 15 read intervals ----

def test_everything_at_once_on_the_full_array():
    """cfg2, exposure 0 (the first tried: no undecided flag), float32 reads, one upload per slot: rejection, variances, 256
    channels over a hull of 384 columns that ends with the frame, the optimal extraction and the optimal channels -- the
    largest spectra block the ABI delivers.  The time spent in the numpy laws is printed beside the test's own."""
    t_start = time.time()
    v = tfp.visit("cfg2")
    ctx = tfp.engine_of(v).ctx
    pl = tfp.planes_of(v)
    S, R, H = pl.S, v.NSAMP - 1, 8
    assert (S, R) == (1024, 15)
    over = over_of(v)
    windows = tfp.descriptor(v, 0, extraction.ExtractionOptions(), **over)[1].extraction_plan.row_windows
    edges = A_UM + PX_UM * (S - 384 + 1.5 * np.arange(257))
    ch, sol = extraction.Channels(edges), (np.full(S, A_UM), np.full(S, PX_UM))
    prof = extraction.Profile(tfp.made_up_profile(windows, S), fpl.heights(windows))

    def plan_of(supplied):
        return extraction.Extraction(windows, crrej=True, channels=ch, row_solution=sol, variance=extraction.Variances(RN),
                                     optimal=extraction.Optimal(H, profile=prof if supplied else None, channels=True))

    own, fixed = plan_of(False), plan_of(True)
    assert own.hull == (S - 384, S) and ch.n == 256
    desc, _ = tfp.descriptor(v, 0, own, **over)
    for slot in (0, 1):                                              # the two streams
        ctx.upload(slot, desc)
        ctx.run(slot)
    reads = ctx.download(0)
    down = [tfp.every_product(ctx, slot, *ctx.download_spectra(slot)) for slot in (0, 1)]
    t_law = time.time()
    c = check(ctx, 0, v, own, reads, "cfg2 own profile")
    t_law = time.time() - t_law
    assert c.rejected.sum() > 0 and int(c.mask.max()) >> 8 > 0
    assert_the_far_channels_are_lit(c, "cfg2")
    assert_the_far_optimal_channels_are_lit(c, "cfg2 own profile")
    ok = c.want_optimal.ok
    assert ok[:, 512:].any() and (~ok[:, 512:]).any() and ok[5:].any()
    # the whole block lies where the layout says, and the pinned path brings the bytes of the blocking one, in either slot
    want, total = sll.layout(S, R, crrej=True, C=256, variance=True, optimal=True, optimal_channels=True)
    assert sorted(want) == sorted(tfp.PRODUCTS)
    for slot in (0, 1):
        ctx.fetch_spectra_async(slot)
        spectra, sky = ctx.wait_spectra(slot)
        at = tfp.pinned_addresses(ctx, slot, spectra, sky)
        assert {name: at[name] - at["spectra"] for name in tfp.PRODUCTS} == want, slot
        pinned = tfp.every_product(ctx, slot, spectra, sky)
        for name in tfp.PRODUCTS:
            assert pinned[name].tobytes() == down[slot][name].tobytes() == down[0][name].tobytes(), (slot, name)
            assert down[0][name].any(), name
    ctx.run(1)                                                       # a second run sums again, it does not add
    again = tfp.every_product(ctx, 1, *ctx.download_spectra(1))
    for name in tfp.PRODUCTS:
        assert again[name].tobytes() == down[0][name].tobytes(), name
    # the supplied profile
    run_plan(ctx, 0, fixed)
    t0 = time.time()
    f = check(ctx, 0, v, fixed, reads, "cfg2 supplied profile", box=False)
    t_law += time.time() - t0
    assert_the_far_optimal_channels_are_lit(f, "cfg2 supplied profile")
    assert f.spectra.tobytes() == c.spectra.tobytes() and f.optimal.tobytes() != c.optimal.tobytes()
    print("caps: cfg2: %.1f s in all, %.1f s of them in the numpy laws" % (time.time() - t_start, t_law))
