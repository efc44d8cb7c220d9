"""GPU: the profile planes (wayne_exposure_deliver_profile, k_extract_profile) and the optimal extraction with a supplied
profile (wayne_exposure_set_optimal_profile, k_extract_optimal_fixed).

The oracle in every parity case is the law restated in numpy (tests/fixed_profile_law.py) applied to the reads of the SAME
slot and to the box arrays the SAME slot delivered.  The planes are the same left-to-right sums of the same numbers: equal
to the bit.  With a supplied profile only the order of the row sums differs: optimal_law's derived bounds (2e-9 M_U / W,
4e-9 of the variance, fallback columns to the bit).  Host side, and the same ensemble on CPU-oracle reads:
tests/test_fixed_profile.py."""
import collections
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import channel_law
import crrej_law
import extraction_law as law
import fixed_profile_law as fpl
import helpers
import optimal_law
import spectra_layout_law as sll
from wayne_amd import _lib, engine, extraction, run_visit
from wayne_amd.visit import VisitRunner

pytestmark = pytest.mark.gpu

_visits, _planes = {}, {}
Run = collections.namedtuple("Run", "reads spectra sky spectra_var sky_var optimal optimal_var planes plan")
RN = 20.0
HALF_WIDTHS = (1, 16)


def visit(name, n=6):
    if (name, n) not in _visits:
        _visits[(name, n)] = helpers.make_visit(name, n_exposures=n)
    return _visits[(name, n)]


def planes_of(v):
    if v.name not in _planes:
        _planes[v.name] = law.Planes(v)
    return _planes[v.name]


def engine_of(v):
    return engine.get_engine(0, v.grism, v.detector, v.calibration, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)


def descriptor(v, i, ex, out_dtype=np.float32, **over):
    gen = helpers.product_generator(v, i)
    return gen.build_descriptor(engine_of(v), out_dtype=out_dtype, extraction=ex, **v.frame_kwargs(i, **over)), gen


def fetch(ctx, slot, plan, reads=True):
    r = ctx.download(slot) if reads else None
    spectra, sky = ctx.download_spectra(slot)
    sv, kv, _ = ctx.variances(slot)
    op, ov = ctx.optimal(slot)
    return Run(r, spectra, sky, sv, kv, op, ov, ctx.profile_planes(slot) if ctx.delivers_profile(slot) else None, plan)


def crrej_of(plan):
    return (plan.crrej.k, plan.crrej.read_noise) if plan.crrej is not None else None


def made_up_profile(windows, S, seed=7):
    """A profile no exposure made: per window a Gaussian along the window's rows whose centre and width drift with the
    column, normalised per column, then -- so that every branch of the law is taken -- ripples that go below zero on the
    wings (the clamp), columns of zeros (W = 0: the box values) and columns that do not sum to 1."""
    rs = np.random.RandomState(seed)
    rows = fpl.heights(windows)
    out = np.zeros((sum(rows), S))
    at = 0
    x = np.arange(S)[None, :]
    for h in rows:
        y = np.arange(h)[:, None]
        g = np.exp(-0.5 * ((y - 0.5 * h - 2.0 * np.sin(x / 40.0)) / (0.12 * h + 0.5 + 0.002 * x)) ** 2)
        g = g / g.sum(axis=0) - 0.02 / h * (1.0 + np.cos(3.0 * y + x))
        g = g * (1.0 + 0.05 * rs.standard_normal((1, S)))
        g[:, rs.random_sample(S) < 0.05] = 0.0
        out[at:at + h] = g
        at += h
    return out


def assert_planes_are_the_law(run, v, H, what, reads=None):
    plan = run.plan
    want = fpl.planes(run.reads if reads is None else reads, planes_of(v), plan.row_windows, H, run.sky, plan.steps, crrej_of(plan))
    assert run.planes.shape == want.shape and run.planes.dtype == np.float64, what
    assert run.planes.tobytes() == want.tobytes(), "%s: planes differ by up to %g" % (what, np.abs(run.planes - want).max())
    return want


def assert_is_the_fixed_law(run, v, H, profile, what, reads=None, both=True):
    plan = run.plan
    want = fpl.restate(run.reads if reads is None else reads, planes_of(v), plan.row_windows, H, plan.variance.read_noise,
                       profile, run.spectra, run.sky, run.spectra_var, run.sky_var, plan.steps, crrej_of(plan))
    optimal_law.assert_parity(run.optimal, run.optimal_var, want, run.spectra, run.spectra_var, what)
    R = v.NSAMP - 1
    if both:
        assert want.ok.any() and (~want.ok[:R]).any(), what
    return want


def busy_rate(v, per_interval=30.0):
    dt = np.diff(np.concatenate([[0.0], np.asarray(v.read_times, dtype=float)]))
    N = v.detector.light_sensitive_size(v.SUBARRAY)
    return per_interval * 1024.0 ** 2 / (N * N * dt.min())


VISITS = [("tiny", 0), ("tiny_g102", 0), ("tiny128", 0), ("small256", 1), ("stare256", 0)]
# (tests/test_optimal_gpu.py: the three small visits' star is too faint for ok(x); 30 times brighter both branches are taken)
BRIGHTER = {"tiny": 30.0, "tiny_g102": 30.0, "tiny128": 30.0}


@pytest.mark.parametrize("crrej", [False, True], ids=["plain", "crrej"])
@pytest.mark.parametrize("out_dtype", [np.float32, np.float64, np.uint16], ids=["f32", "f64", "u16"])
@pytest.mark.parametrize("name,i", VISITS, ids=[n for n, _ in VISITS])
def test_planes_and_the_supplied_profile_are_their_laws(name, i, out_dtype, crrej):
    """One upload; per half width one run that delivers the planes AND extracts with a made-up profile."""
    v = visit(name)
    S = planes_of(v).S
    margin = 40 if name in ("tiny", "tiny_g102") else extraction.ROW_MARGIN
    ex = extraction.ExtractionOptions(margin=margin, crrej=crrej or None, variance=extraction.Variances(RN), optimal=True)
    over = dict(cosmic_rate=busy_rate(v) if name.startswith("tiny") else busy_rate(v, 3.0)) if crrej else {}
    if name in BRIGHTER:
        over["stellar_flux"] = np.asarray(v.stellar_flux) * BRIGHTER[name]
    what = "%s[%d] %s crrej %d" % (name, i, np.dtype(out_dtype).name, crrej)
    ctx = engine_of(v).ctx
    desc, gen = descriptor(v, i, ex, out_dtype, **over)
    ctx.upload(0, desc)
    plan = gen.extraction_plan
    prof = extraction.Profile(made_up_profile(plan.row_windows, S), fpl.heights(plan.row_windows))
    reads, runs = None, []
    for H in HALF_WIDTHS:
        ctx.set_optimal(0, extraction.Optimal(H, profile=prof, deliver_profile=True))
        ctx.run(0)
        run = fetch(ctx, 0, plan, reads=reads is None)
        reads = run.reads if reads is None else reads
        if crrej and not runs:
            cr = plan.crrej
            mask = crrej_law.restate(reads, planes_of(v), plan.row_windows, plan.bg_cols, plan.steps, cr.k, cr.read_noise).mask
            assert (ctx.download_crmask(0) == mask).all(), what
        assert_planes_are_the_law(run, v, H, "%s H %d" % (what, H), reads)
        want = assert_is_the_fixed_law(run, v, H, prof.planes, "%s H %d" % (what, H), reads)
        zero = ~prof.planes[:prof.rows[0]].any(axis=0)
        assert zero.any() and not want.ok[0][zero].any(), what           # a column of zeros keeps the box values
        runs.append(run)
    assert runs[0].planes.tobytes() != runs[1].planes.tobytes()           # the planes see the half width ...
    assert runs[0].spectra.tobytes() == runs[1].spectra.tobytes()         # ... the box extraction does not
    if name in ("tiny", "tiny_g102"):
        assert S == 74                                                   # a partial last tile; X(x) is clamped in tile 0
    if name == "small256":
        rows = prof.rows[-1]
        assert rows > 2 * 32 and rows % 32 != 0                          # several chunks and a remainder


def test_an_exposures_own_planes_make_its_profile():
    """The round trip a visit makes: planes delivered, summed and normalised by ProfileSum, supplied again."""
    v = visit("small256")
    ctx = engine_of(v).ctx
    H = 8
    desc, gen = descriptor(v, 1, extraction.ExtractionOptions(variance=extraction.Variances(RN),
                                                              optimal=extraction.Optimal(H, deliver_profile=True)))
    plan = gen.extraction_plan
    ctx.upload(0, desc)
    ctx.run(0)
    own = fetch(ctx, 0, plan)
    assert_planes_are_the_law(own, v, H, "own planes")
    optimal_law.assert_parity(own.optimal, own.optimal_var,
                              optimal_law.restate(own.reads, planes_of(v), plan.row_windows, H, RN, own.spectra, own.sky,
                                                  own.spectra_var, own.sky_var), own.spectra, own.spectra_var, "delivery changes nothing")
    prof = extraction.ProfileSum().add(plan, own.planes).profile()
    assert prof.planes.tobytes() == fpl.normalise(own.planes, plan.row_windows).tobytes() and prof.exposures == 1
    ctx.set_optimal(0, extraction.Optimal(H, profile=prof))
    assert not ctx.delivers_profile(0)
    ctx.run(0)
    fixed = fetch(ctx, 0, plan, reads=False)
    want = assert_is_the_fixed_law(fixed, v, H, prof.planes, "own profile", own.reads)
    # sum_y S1 = S0: where the exposure's own profile is used twice the two extractions agree closely, not to the bit
    ok = want.ok[3] & (own.optimal[3] != own.spectra[3])
    assert ok.sum() > 100
    assert np.abs(fixed.optimal[3][ok] / own.optimal[3][ok] - 1.0).max() < 1e-6


def test_steps_off_and_short_windows():
    v = visit("small256")
    R, S = v.NSAMP - 1, planes_of(v).S
    ctx = engine_of(v).ctx

    def one(ex_of, what):
        desc, gen = descriptor(v, 1, ex_of(extraction.Optimal(8)))
        plan = gen.extraction_plan
        prof = extraction.Profile(made_up_profile(plan.row_windows, S), fpl.heights(plan.row_windows))
        desc, gen = descriptor(v, 1, ex_of(extraction.Optimal(8, profile=prof, deliver_profile=True)))
        ctx.upload(0, desc)
        ctx.run(0)
        run = fetch(ctx, 0, gen.extraction_plan)
        assert_planes_are_the_law(run, v, 8, what)
        assert_is_the_fixed_law(run, v, 8, prof.planes, what)
        return run, prof

    for steps in (extraction.ALL & ~extraction.SKY, extraction.ALL & ~extraction.LAST_READ):
        run, prof = one(lambda o: extraction.ExtractionOptions(steps=steps, variance=True, optimal=o), "steps %d" % steps)
        if not steps & extraction.LAST_READ:                               # a product that is not formed: zeros
            assert not run.planes[-prof.rows[R]:].any() and run.planes[:-prof.rows[R]].any()
            assert not run.optimal[R].any() and not run.optimal_var[R].any() and run.optimal[:R].any()
    full = descriptor(v, 1, extraction.ExtractionOptions(variance=True, optimal=True))[1].extraction_plan
    mid = (full.row_windows[:, 0] + full.row_windows[:, 1]) // 2
    short = [(int(m) - lo, int(m) + hi) for m, (lo, hi) in zip(mid, [(1, 2), (0, 1), (3, 4), (2, 3)])]      # 3, 1, 7 and 5 rows
    run, prof = one(lambda o: extraction.Extraction(short, variance=extraction.Variances(RN), optimal=o), "windows shorter than 8 rows")
    assert prof.rows == (3, 1, 7, 5) and run.planes.shape == (16, S)


def test_the_same_exposure_gives_the_same_bytes():
    v = visit("small256")
    ctx = engine_of(v).ctx
    S = planes_of(v).S
    plan = descriptor(v, 1, extraction.ExtractionOptions(variance=True, optimal=True))[1].extraction_plan
    prof = extraction.Profile(made_up_profile(plan.row_windows, S), fpl.heights(plan.row_windows))
    opts = extraction.ExtractionOptions(crrej=True, variance=True, optimal=extraction.Optimal(8, profile=prof, deliver_profile=True))
    desc, gen = descriptor(v, 1, opts, cosmic_rate=busy_rate(v, 3.0))
    plan = gen.extraction_plan
    for slot in (0, 1):                                              # the two streams
        ctx.upload(slot, desc)
        ctx.run(slot)
    a, b = fetch(ctx, 0, plan), fetch(ctx, 1, plan)
    for name in ("optimal", "optimal_var", "planes", "spectra"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert a.optimal.max() > 1e4 and a.optimal.tobytes() != a.spectra.tobytes()
    other, _ = descriptor(v, 0, extraction.ExtractionOptions(margin=3, variance=extraction.Variances(5.0),
                                                             optimal=extraction.Optimal(3, deliver_profile=True)))
    ctx.upload(0, other)                                             # another exposure with another plan in between
    ctx.run(0)
    ctx.synchronize()
    ctx.upload(3, desc)
    ctx.run(3)
    c = fetch(ctx, 3, plan)
    ctx.run(3)                                                       # a second run sums again, it does not add
    d = fetch(ctx, 3, plan)
    for name in ("optimal", "optimal_var", "planes"):
        assert getattr(c, name).tobytes() == getattr(a, name).tobytes() == getattr(d, name).tobytes(), name
    # the delivery path: the spectra's pinned copy, then the planes' own
    ctx.fetch_spectra_async(3)
    ctx.wait_spectra(3)
    ctx.fetch_profile(3)
    assert ctx.optimal(3)[0].tobytes() == a.optimal.tobytes() and ctx.profile_planes(3).tobytes() == a.planes.tobytes()


def test_off_means_off_and_what_clears_optimal_clears_the_profile():
    v = visit("small256")
    ctx = engine_of(v).ctx
    S = planes_of(v).S
    desc, gen = descriptor(v, 1, extraction.ExtractionOptions(variance=True, optimal=True))
    plan = gen.extraction_plan
    ctx.upload(0, desc)
    ctx.run(0)
    spectra, _ = ctx.download_spectra(0)
    plain = ctx.optimal(0)
    for call in (ctx.fetch_profile, ctx.profile_planes):              # nothing to fetch without delivery
        with pytest.raises(_lib.WayneError) as e:
            call(0)
        assert e.value.status == _lib.E_STATE
    prof = extraction.Profile(made_up_profile(plan.row_windows, S), fpl.heights(plan.row_windows))
    ctx.set_optimal_profile(0, prof)
    ctx.deliver_profile(0)
    with pytest.raises(_lib.WayneError) as e:                        # delivery is on, but no run has written the planes
        ctx.fetch_profile(0)
    assert e.value.status == _lib.E_STATE
    ctx.run(0)
    with pytest.raises(_lib.WayneError) as e:                        # ... and nobody has settled the run
        ctx.fetch_profile(0)
    assert e.value.status == _lib.E_STATE
    assert ctx.download_spectra(0)[0].tobytes() == spectra.tobytes()
    assert ctx.optimal(0)[0].tobytes() != plain[0].tobytes() and ctx.profile_planes(0).any()
    # cleared one by one: the exposure's own profile again, to the bit
    ctx.set_optimal_profile(0, None)
    ctx.deliver_profile(0, on=False)
    ctx.run(0)
    ctx.download_spectra(0)
    assert ctx.optimal(0)[0].tobytes() == plain[0].tobytes() and ctx.optimal(0)[1].tobytes() == plain[1].tobytes()
    # set_optimal, set_variance, set_extraction and upload clear both
    for clear in (lambda: ctx.set_optimal(0, True), lambda: (ctx.set_variance(0, True), ctx.set_optimal(0, True)),
                  lambda: ctx.set_extraction(0, plan), lambda: ctx.upload(0, desc)):
        ctx.set_optimal_profile(0, prof)
        ctx.deliver_profile(0)
        clear()
        assert ctx.has_optimal(0) and not ctx.delivers_profile(0)
        ctx.run(0)
        ctx.download_spectra(0)
        assert ctx.optimal(0)[0].tobytes() == plain[0].tobytes()
        assert ctx._L.wayne_exposure_fetch_profile(ctx._h, 0) == _lib.E_STATE
    # without the optimal extraction there is nothing to attach them to
    ctx.set_optimal(0, None)
    rows = (C.c_int * 4)(*prof.rows)
    assert ctx._L.wayne_exposure_deliver_profile(ctx._h, 0, 1) == _lib.E_STATE
    assert ctx._L.wayne_exposure_set_optimal_profile(ctx._h, 0, prof.planes.ctypes.data_as(_lib._dp), rows) == _lib.E_STATE


def test_a_profile_of_other_window_heights_is_refused_at_run_and_the_slot_stays_usable():
    v = visit("small256")
    ctx = engine_of(v).ctx
    S = planes_of(v).S
    desc, gen = descriptor(v, 1, extraction.ExtractionOptions(variance=True, optimal=True))
    plan = gen.extraction_plan
    rows = fpl.heights(plan.row_windows)
    good = extraction.Profile(made_up_profile(plan.row_windows, S), rows)
    ctx.upload(0, desc)
    ctx.set_optimal_profile(0, good)
    ctx.run(0)
    want = fetch(ctx, 0, plan, reads=False)
    taller = [(lo, hi + 1) for lo, hi in plan.row_windows]
    bad = extraction.Profile(made_up_profile(taller, S), fpl.heights(taller))
    ctx.set_optimal_profile(0, bad)                                  # accepted: heights a window can have ...
    with pytest.raises(_lib.WayneError) as e:
        ctx.run(0)                                                   # ... but not this slot's
    assert e.value.status == _lib.E_INVALID and "window heights" in str(e.value)
    assert ctx._L.wayne_exposure_run(ctx._h, 0) == _lib.E_INVALID
    ctx.set_optimal_profile(0, good)
    ctx.run(0)
    again = fetch(ctx, 0, plan, reads=False)
    assert again.optimal.tobytes() == want.optimal.tobytes() and again.optimal_var.tobytes() == want.optimal_var.tobytes()
    # heights no window can have are refused when they are set: the slot keeps extracting with its own profile
    for wrong in ((0,) + rows[1:], rows[:3] + (S + 1,), (-1,) + rows[1:]):
        arr = (C.c_int * 4)(*wrong)
        assert ctx._L.wayne_exposure_set_optimal_profile(ctx._h, 0, good.planes.ctypes.data_as(_lib._dp), arr) == _lib.E_INVALID
    assert ctx._L.wayne_exposure_set_optimal_profile(ctx._h, 0, good.planes.ctypes.data_as(_lib._dp), None) == _lib.E_INVALID
    ctx.run(0)
    ctx.download_spectra(0)
    ctx.set_optimal_profile(0, None)
    ctx.run(0)
    ctx.download_spectra(0)
    assert ctx.optimal(0)[0].tobytes() != want.optimal.tobytes()


class SameExposure(VisitRunner):
    """Every index is exposure 0 of the visit with the index's own random draws: no cosmic rays, no scan-speed variation,
    no flat (the set-up of tests/test_optimal_gpu.py's ensemble)."""

    def frame_kwargs(self, i):
        return self.visit.frame_kwargs(0, cosmic_rate=None, ssv_generator=None, add_flat=False)


def test_a_visits_profile_gives_trustworthy_channel_sums_on_the_devices_reads():
    """The ensemble of tests/test_fixed_profile.py on device reads, through VisitRunner: the profile from exposures 32 ..
    47 (build_profile), exposures 0 .. 31 extracted with it and with their own profiles, 10 channels of 13 whole columns, H
    = 8; the assertions of fixed_profile_law.assert_ensemble on the last-read product, every interval printed.  The
    predicted variance of a channel takes the sky level's share once per channel, for which it needs W and G per column:
    the device delivers 1 / W + (G/W)^2 sky_var only, so W and G are the numpy law's on the device's own reads and box arrays
    (the parity tests above hold them to 1e-9 of the device's)."""
    v = visit("small256")
    n, H = 32, 8
    R, pl = v.NSAMP - 1, planes_of(v)
    runner = SameExposure(v)
    base = extraction.ExtractionOptions(variance=extraction.Variances(RN), optimal=extraction.Optimal(H))
    profiles = runner.build_profile(range(n, n + 16), base)
    (key, prof), = profiles.items()
    assert prof.exposures == 16 and key == (prof.rows, 1)
    kept = runner.run(range(n), keep=True, extraction=base)
    own_optimal = np.array([runner.optimal[i] for i in range(n)])
    spectra = np.array([kept[i][1] for i in range(n)])
    fixed_opts = extraction.ExtractionOptions(variance=extraction.Variances(RN), optimal=extraction.Optimal(H, profile=profiles))
    spectra2, _ = runner.run_spectra(range(n), extraction=fixed_opts)
    assert spectra2.tobytes() == spectra.tobytes() and runner.optimal.tobytes() != own_optimal.tobytes()
    assert runner.profile_planes is None and runner.plans[0].optimal.profile is prof
    windows = runner.plans[0].row_windows
    pred_own, pred_fixed = np.zeros((n, R + 1, fpl.N_CHANNELS)), np.zeros((n, R + 1, fpl.N_CHANNELS))
    for i in range(n):
        box = (kept[i][1], kept[i][2], runner.spectra_var[i], runner.sky_var[i])
        o = optimal_law.restate(kept[i][0], pl, windows, H, RN, *box)
        f = fpl.restate(kept[i][0], pl, windows, H, RN, prof.planes, *box)
        for p in range(R + 1):
            pred_own[i, p] = fpl.channel_variance(o, p, box[2], box[3])
            pred_fixed[i, p] = fpl.channel_variance(f, p, box[2], box[3])
        if i == 0:
            assert f.ok[R, fpl.CHANNEL_COLS[0]:fpl.CHANNEL_COLS[1]].all() and o.ok[R, fpl.CHANNEL_COLS[0]:fpl.CHANNEL_COLS[1]].all()
    for p in list(range(R)) + [R]:
        fixed = fpl.channel_figures(runner.optimal[:, p], pred_fixed[:, p], spectra[:, p])
        own = fpl.channel_figures(own_optimal[:, p], pred_own[:, p], spectra[:, p])
        print("device, %d exposures, %s: channel variance / box: supplied profile %.3f, own profile %.3f; ensemble / predicted: "
              "%.3f, %.3f; bias %+.2e (5 sd: %.1e), %+.2e" % (n, "last read" if p == R else "interval %d" % p, fixed[0], own[0],
                                                             fixed[1], own[1], fixed[2], fixed[3], own[2]))
    fpl.assert_ensemble(fixed, own, n, "device")


def test_frames_and_visits_carry_the_planes():
    v = visit("tiny")
    opt = extraction.Optimal(8, deliver_profile=True)
    exp = helpers.product_generator(v, 0).scanning_frame(extraction=True, variance=True, optimal=opt, **v.frame_kwargs(0))
    rows = fpl.heights(exp.extraction.row_windows)
    assert exp.profile_planes.shape == (sum(rows), 74) and exp.profile_planes.any()
    plain = helpers.product_generator(v, 0).scanning_frame(extraction=True, variance=True, optimal=True, **v.frame_kwargs(0))
    assert not hasattr(plain, "profile_planes") and plain.optimal.tobytes() == exp.optimal.tobytes()
    prof = extraction.ProfileSum().add(exp.extraction, exp.profile_planes).profile()
    again = helpers.product_generator(v, 0).scanning_frame(extraction=True, variance=True, optimal=extraction.Optimal(8, profile=prof),
                                                           **v.frame_kwargs(0))
    assert again.extraction.optimal.profile is prof and again.spectra.tobytes() == exp.spectra.tobytes()
    runner = VisitRunner(v)
    opts = extraction.ExtractionOptions(variance=True, optimal=opt)
    runner.run_spectra(range(2), extraction=opts)
    assert len(runner.profile_planes) == 2 and runner.profile_planes[0].tobytes() == exp.profile_planes.tobytes()
    runner.run(range(2), extraction=opts)
    assert sorted(runner.profile_planes) == [0, 1] and runner.profile_planes[0].tobytes() == exp.profile_planes.tobytes()
    runner.run_spectra(range(1), extraction=extraction.ExtractionOptions(variance=True, optimal=True))
    assert runner.profile_planes is None


def test_a_slot_copies_a_profile_it_already_holds_only_once():
    """A visit hands the same Profile to a slot with every exposure it uploads there."""
    v = visit("small256")
    ctx = engine_of(v).ctx
    S = planes_of(v).S
    plan = descriptor(v, 1, extraction.ExtractionOptions(variance=True, optimal=True))[1].extraction_plan
    prof = extraction.Profile(made_up_profile(plan.row_windows, S, seed=11), fpl.heights(plan.row_windows))
    desc, gen = descriptor(v, 1, extraction.ExtractionOptions(variance=True, optimal=extraction.Optimal(8, profile=prof)))
    n0 = ctx.profile_uploads()
    ctx.upload(5, desc)
    ctx.run(5)
    first = fetch(ctx, 5, plan)
    assert ctx.profile_uploads() == n0 + 1
    for _ in range(3):                                               # upload clears the option; the device copy stays
        ctx.upload(5, desc)
        ctx.run(5)
        again = fetch(ctx, 5, plan, reads=False)
        assert again.optimal.tobytes() == first.optimal.tobytes() and again.optimal_var.tobytes() == first.optimal_var.tobytes()
    assert ctx.profile_uploads() == n0 + 1
    assert_is_the_fixed_law(first, v, 8, prof.planes, "held profile")
    # one value of one pixel changed: copied, and the column's result follows it
    changed = prof.planes.copy()
    col = int(np.argmax(first.optimal[3] != first.spectra[3]))
    changed[sum(prof.rows[:3]) + prof.rows[3] // 2, col] *= 1.5
    ctx.set_optimal_profile(5, extraction.Profile(changed, prof.rows))
    ctx.run(5)
    other = fetch(ctx, 5, plan, reads=False)
    assert ctx.profile_uploads() == n0 + 2 and other.optimal[3, col] != first.optimal[3, col]
    assert_is_the_fixed_law(other, v, 8, changed, "changed profile", first.reads)
    # the other heights of the same number of values: copied too (the heights are part of what a slot holds)
    ctx.set_optimal_profile(5, prof)
    assert ctx.profile_uploads() == n0 + 3
    swapped = extraction.Profile(prof.planes, (prof.rows[1], prof.rows[0]) + prof.rows[2:])
    ctx.set_optimal_profile(5, swapped)
    assert ctx.profile_uploads() == n0 + (4 if swapped.rows != prof.rows else 3)


def test_the_cli_forms_the_visits_profiles_in_a_first_pass(tmp_path):
    work = str(tmp_path / "visit")
    shutil.copytree(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures", "mini_visit"), work)
    yml = os.path.join(work, "params.yml")
    out, own = str(tmp_path / "fixed.npz"), str(tmp_path / "own.npz")
    common = ["-p", yml, "--max-exposures", "4", "--variances", "--optimal", "5"]
    obs = run_visit.run(common + ["--spectra-only", out, "--optimal-profile", "2"])
    z = np.load(out)
    assert int(z["optimal_profile_exposures"]) == 2 and z["optimal"].shape == z["spectra"].shape
    keys = [extraction.profile_key(p, obs.scan_speed if obs.spatial_scan else 0.0) for p in obs.spectra_result["plans"]]
    assert set(keys) == set(obs.optimal_profiles)                      # every group of the visit has its profile
    for key, prof in obs.optimal_profiles.items():
        assert prof.exposures == min(2, keys.count(key)) and prof.rows == key[0]
    for plan, key in zip(obs.spectra_result["plans"], keys):
        assert plan.optimal.profile is obs.optimal_profiles[key] and plan.optimal.half_width == 5
    run_visit.run(common + ["--spectra-only", own])
    zo = np.load(own)
    assert "optimal_profile_exposures" not in zo.files and sorted(set(z.files) - set(zo.files)) == ["optimal_profile_exposures"]
    assert zo["spectra"].tobytes() == z["spectra"].tobytes() and zo["spectra_var"].tobytes() == z["spectra_var"].tobytes()
    assert zo["optimal"].tobytes() != z["optimal"].tobytes()
    # the file's values are the law applied with the group's profile: exposure 0 through the frame API, reads and all
    obs.spectra_out, obs.spectra_only = None, False
    frame = obs._generate_exposure(obs.exp_start_times[0], 1, write_fits=False)
    assert frame.optimal.tobytes() == z["optimal"][0].tobytes() and frame.extraction.optimal.profile is obs.optimal_profiles[keys[0]]


# ---- the optimal channels (wayne_exposure_set_optimal_channels; k_extract_bins_opt and k_extract_bins_opt_finish) ----

WIDE = {"G141": (1.0, 1.8), "G102": (0.7, 1.25)}          # beyond the first order at both ends
_flats = {}


def flat_of(v):
    if v.name not in _flats:
        _flats[v.name] = channel_law.Flat(v)
    return _flats[v.name]


def channel_oracle(run, v, H, profile, reads=None, mutate=None):
    plan = run.plan
    return fpl.channels(run.reads if reads is None else reads, planes_of(v), plan.row_windows, H, plan.variance.read_noise, profile,
                        run.spectra, run.sky, run.spectra_var, run.sky_var, plan.channels.edges_um, plan.row_solution[0],
                        plan.row_solution[1], plan.steps, flat_of(v) if plan.channels.flat else None, crrej_of(plan), mutate)


@pytest.mark.parametrize("flat", [False, True], ids=["noflat", "flat"])
@pytest.mark.parametrize("crrej", [False, True], ids=["plain", "crrej"])
@pytest.mark.parametrize("out_dtype", [np.float32, np.float64, np.uint16], ids=["f32", "f64", "u16"])
@pytest.mark.parametrize("name,i", VISITS, ids=[n for n, _ in VISITS])
def test_optimal_channels_are_their_law_with_either_profile(name, i, out_dtype, crrej, flat):
    """One upload; per half width a run with the exposure's own profile and one with a made-up supplied profile."""
    v = visit(name)
    S, R = planes_of(v).S, v.NSAMP - 1
    margin = 40 if name in ("tiny", "tiny_g102") else extraction.ROW_MARGIN
    ch = extraction.Channels.linear(*WIDE[v.grism.name], 20).with_flat(flat)
    ex = extraction.ExtractionOptions(margin=margin, channels=ch, crrej=crrej or None, variance=extraction.Variances(RN), optimal=True)
    over = dict(cosmic_rate=busy_rate(v) if name.startswith("tiny") else busy_rate(v, 3.0)) if crrej else {}
    if name in BRIGHTER:
        over["stellar_flux"] = np.asarray(v.stellar_flux) * BRIGHTER[name]
    what = "%s[%d] %s crrej %d flat %d" % (name, i, np.dtype(out_dtype).name, crrej, flat)
    ctx = engine_of(v).ctx
    desc, gen = descriptor(v, i, ex, out_dtype, **over)
    ctx.upload(0, desc)
    plan = gen.extraction_plan
    prof = extraction.Profile(made_up_profile(plan.row_windows, S), fpl.heights(plan.row_windows))
    reads, box_channels = None, None
    for H in HALF_WIDTHS:
        for supplied in (None, prof):
            ctx.set_optimal(0, extraction.Optimal(H, profile=supplied, channels=True))
            assert ctx.has_optimal_channels(0)
            ctx.run(0)
            run = fetch(ctx, 0, plan, reads=reads is None)
            reads = run.reads if reads is None else reads
            got, got_var = ctx.optimal_channels(0)
            assert got.shape == got_var.shape == (R + 1, 20) and got.dtype == np.float64
            want = channel_oracle(run, v, H, None if supplied is None else prof.planes, reads)
            fpl.assert_channel_parity(got, got_var, want, "%s H %d %s profile" % (what, H, "own" if supplied is None else "supplied"))
            assert want.ok.any() and (~want.ok).any()                  # both branches of e, k and ev
            if name == "small256" and not crrej and out_dtype == np.float32:
                # the hand mutations of the law are seen by the parity bound: w in place of w^2, K^2 sky_var dropped
                for mutate in ("w", "no_sky"):
                    with pytest.raises(AssertionError):
                        fpl.assert_channel_parity(got, got_var, channel_oracle(run, v, H, None if supplied is None else prof.planes,
                                                                               reads, mutate), what + " mutated: " + mutate)
            box_channels = ctx.channels(0) if box_channels is None else box_channels
            assert ctx.channels(0).tobytes() == box_channels.tobytes()  # the box channels do not see any of it


def whole_column_plan(v, i=1):
    """small256's default windows with 10 channels of 13 whole columns (59 .. 188), one solution for all rows, the flat off."""
    S = planes_of(v).S
    base = descriptor(v, i, extraction.ExtractionOptions(variance=True, optimal=True))[1].extraction_plan
    a, b = 1.0, 0.00390625                                         # 2^-8: a + b x and (e - a) / b are exact
    sol = (np.full(S, a), np.full(S, b))
    edges = np.array([59 + 13 * k for k in range(11)], dtype=np.float64)
    # edges that land on whole columns EXACTLY: (e - a) / b must give the integer back
    edges_um = a + b * edges
    assert ((edges_um - a) / b == edges).all()
    return base, extraction.Channels(edges_um, flat=False), sol


def test_with_whole_column_edges_the_channels_are_the_slots_own_optimal_summed():
    v = visit("small256")
    ctx = engine_of(v).ctx
    S, R, H = planes_of(v).S, v.NSAMP - 1, 8
    base, ch, sol = whole_column_plan(v)
    prof = extraction.Profile(made_up_profile(base.row_windows, S), fpl.heights(base.row_windows))
    for supplied in (None, prof):
        plan = extraction.Extraction(base.row_windows, channels=ch, row_solution=sol, variance=extraction.Variances(RN),
                                     optimal=extraction.Optimal(H, profile=supplied, channels=True))
        desc, _ = descriptor(v, 1, plan)
        ctx.upload(0, desc)
        ctx.run(0)
        run = fetch(ctx, 0, plan)
        got, got_var = ctx.optimal_channels(0)
        want = channel_oracle(run, v, H, None if supplied is None else prof.planes)
        fpl.assert_channel_parity(got, got_var, want, "whole columns")
        summed = fpl.channel_sums(run.optimal)
        assert (np.abs(got - summed) <= fpl.REL * want.M).all()
        # the variance: sum 1 / W plus the sky level's share ONCE -- not the sum of optimal_var
        res = (optimal_law.restate(run.reads, planes_of(v), plan.row_windows, H, RN, run.spectra, run.sky, run.spectra_var, run.sky_var)
               if supplied is None else
               fpl.restate(run.reads, planes_of(v), plan.row_windows, H, RN, prof.planes, run.spectra, run.sky, run.spectra_var, run.sky_var))
        for p in range(R + 1):
            if res.ok[p, 59:189].all():
                once = fpl.channel_variance(res, p, run.spectra_var, run.sky_var)
                assert (np.abs(got_var[p] - once) <= 4 * fpl.REL * once).all()
                assert (got_var[p] > fpl.channel_sums(run.optimal_var[p]) * (1 + 1e-6)).all()
        if supplied is None:                                         # (the made-up profile has columns of zeros among them)
            assert res.ok[R, 59:189].all()
        # (whole columns have w = w^2: that mutation is shown on the planned channels, in the grid above)
        with pytest.raises(AssertionError):
            fpl.assert_channel_parity(got, got_var, channel_oracle(run, v, H, None if supplied is None else prof.planes, mutate="no_sky"))


def test_optimal_channels_same_bytes_clearing_and_refusals():
    v = visit("small256")
    ctx = engine_of(v).ctx
    S = planes_of(v).S
    ch = extraction.Channels.linear(1.05, 1.75, 23)
    base = descriptor(v, 1, extraction.ExtractionOptions(variance=True, optimal=True))[1].extraction_plan
    prof = extraction.Profile(made_up_profile(base.row_windows, S), fpl.heights(base.row_windows))
    opts = extraction.ExtractionOptions(crrej=True, channels=ch, variance=True, optimal=extraction.Optimal(8, profile=prof, channels=True))
    desc, gen = descriptor(v, 1, opts, cosmic_rate=busy_rate(v, 3.0))
    plan = gen.extraction_plan
    for slot in (0, 1):                                              # the two streams
        ctx.upload(slot, desc)
        ctx.run(slot)
    a, b = fetch(ctx, 0, plan, reads=False), fetch(ctx, 1, plan, reads=False)
    ca, cb = ctx.optimal_channels(0), ctx.optimal_channels(1)
    assert ca[0].tobytes() == cb[0].tobytes() and ca[1].tobytes() == cb[1].tobytes() and a.optimal.tobytes() == b.optimal.tobytes()
    ctx.run(1)                                                       # a second run sums again, it does not add
    ctx.fetch_spectra_async(1)                                       # ... and the pinned copy brings the same bytes
    ctx.wait_spectra(1)
    cc = ctx.optimal_channels(1)
    assert cc[0].tobytes() == ca[0].tobytes() and cc[1].tobytes() == ca[1].tobytes() and ca[0].any() and (ca[1] > 0).all()
    box = ctx.channels(1)
    # off: the arrays in front lie where they lay
    ctx.set_optimal_channels(1, on=False)
    ctx.run(1)
    off = fetch(ctx, 1, plan, reads=False)
    assert off.optimal.tobytes() == a.optimal.tobytes() and ctx.channels(1).tobytes() == box.tobytes()
    with pytest.raises(_lib.WayneError) as e:
        ctx.optimal_channels(1)
    assert e.value.status == _lib.E_STATE
    # set_channels, set_optimal and what clears them clear the option
    for clear in (lambda: ctx.set_channels(1, ch, plan.row_solution), lambda: ctx.set_optimal(1, extraction.Optimal(8, profile=prof))):
        ctx.set_optimal_channels(1)
        assert ctx.has_optimal_channels(1)
        clear()
        assert not ctx.has_optimal_channels(1)
        assert ctx._L.wayne_exposure_optimal_channels(ctx._h, 1, C.byref(_lib._dp()), C.byref(_lib._dp())) == _lib.E_STATE
    # without channels, or without the optimal extraction, there is nothing to bin
    nochan, _ = descriptor(v, 1, extraction.ExtractionOptions(variance=True, optimal=True))
    ctx.upload(2, nochan)
    assert ctx._L.wayne_exposure_set_optimal_channels(ctx._h, 2, 1) == _lib.E_STATE
    noopt, _ = descriptor(v, 1, extraction.ExtractionOptions(channels=ch, variance=True))
    ctx.upload(2, noopt)
    assert ctx._L.wayne_exposure_set_optimal_channels(ctx._h, 2, 1) == _lib.E_STATE
    ctx.run(2)                                                       # ... and the slot extracts as it was told
    ctx.download_spectra(2)
    assert ctx.channels(2).shape == box.shape
    with pytest.raises(ValueError):
        extraction.Extraction(base.row_windows, variance=True, optimal=extraction.Optimal(8, channels=True))


def test_a_visits_profile_gives_trustworthy_channels_on_the_devices_reads():
    """The issue's ensemble on what the device DELIVERS: 32 exposures of small256 that differ in their draws alone (the flat
    off), 10 channels over 1.15 - 1.65 um with the planned slanted row solution, H = 8, the profile from exposures 32 .. 47
    (VisitRunner.build_profile).  channels_opt and channels_opt_var with the visit's profile against the box channels, and
    against the same with the exposures' own profile; fixed_profile_law.assert_ensemble on the last-read product."""
    v = visit("small256")
    n, H = 32, 8
    R = v.NSAMP - 1
    runner = SameExposure(v)
    ch = extraction.Channels.linear(1.15, 1.65, 10).with_flat(False)

    def opts(profile):
        return extraction.ExtractionOptions(channels=ch, variance=extraction.Variances(RN),
                                            optimal=extraction.Optimal(H, profile=profile, channels=True))

    profiles = runner.build_profile(range(n, n + 16), opts(None))
    assert len(profiles) == 1 and list(profiles.values())[0].exposures == 16
    runner.run_spectra(range(n), extraction=opts(None))
    box, box_var = runner.channels, runner.channels_var
    own, own_var = runner.channels_opt, runner.channels_opt_var
    assert own.shape == own_var.shape == box.shape == (n, R + 1, 10)
    runner.run_spectra(range(n), extraction=opts(profiles))
    assert runner.channels.tobytes() == box.tobytes() and runner.channels_opt.tobytes() != own.tobytes()
    for p in list(range(R)) + [R]:
        b = fpl.delivered_figures(box[:, p], box_var[:, p], box[:, p])
        fixed = fpl.delivered_figures(runner.channels_opt[:, p], runner.channels_opt_var[:, p], box[:, p])
        mine = fpl.delivered_figures(own[:, p], own_var[:, p], box[:, p])
        print("device, %d exposures, %s: box ensemble / predicted %.3f; channels_opt variance / box: visit's profile %.3f, own "
              "profile %.3f; ensemble / predicted: %.3f, %.3f; bias %+.2e (5 sd: %.1e), %+.2e" % (
                  n, "last read" if p == R else "interval %d" % p, b[1], fixed[0], mine[0], fixed[1], mine[1], fixed[2], fixed[3], mine[2]))
    fpl.assert_ensemble(fixed, mine, n, "device, delivered channels")


def test_optimal_channels_with_steps_off_and_short_windows():
    """The cases of test_steps_off_and_short_windows for the optimal channels, with either profile source: the sky off (bt =
    k = 0, so K = 0), the last read off (zeros for that product, written by the finish kernel's own branch), and windows of
    3, 1, 7 and 5 rows (three of the four row groups of a chunk hold no row, the staging of d runs on single waves)."""
    v = visit("small256")
    R, S, H = v.NSAMP - 1, planes_of(v).S, 8
    ctx = engine_of(v).ctx
    ch = extraction.Channels.linear(*WIDE[v.grism.name], 20)

    def both_sources(ex_of, what):
        plan = descriptor(v, 1, ex_of(extraction.Optimal(H, channels=True)))[1].extraction_plan
        prof = extraction.Profile(made_up_profile(plan.row_windows, S), fpl.heights(plan.row_windows))
        out = []
        for supplied in (None, prof):
            desc, gen = descriptor(v, 1, ex_of(extraction.Optimal(H, profile=supplied, channels=True)))
            ctx.upload(0, desc)
            ctx.run(0)
            run = fetch(ctx, 0, gen.extraction_plan)
            got, got_var = ctx.optimal_channels(0)
            want = channel_oracle(run, v, H, None if supplied is None else prof.planes)
            fpl.assert_channel_parity(got, got_var, want, "%s, %s profile" % (what, "own" if supplied is None else "supplied"))
            assert want.ok.any() and (~want.ok[:R]).any() and got[:R].any()
            out.append((run, got, got_var, want))
        return out

    no_sky = extraction.ALL & ~extraction.SKY
    for run, got, got_var, want in both_sources(lambda o: extraction.ExtractionOptions(steps=no_sky, channels=ch, variance=True, optimal=o),
                                                "sky off"):
        assert (run.sky == 0.0).all() and (run.sky_var == 0.0).all() and not want.K.any()
        assert got_var.tobytes() != np.zeros_like(got_var).tobytes() and (np.abs(got_var - want.EV) <= 4 * fpl.REL * want.EV).all()
    no_last = extraction.ALL & ~extraction.LAST_READ
    for run, got, got_var, want in both_sources(lambda o: extraction.ExtractionOptions(steps=no_last, channels=ch, variance=True, optimal=o),
                                                "last read off"):
        assert not got[R].any() and not got_var[R].any() and (got_var[:R] > 0.0).all()
        assert not run.optimal[R].any() and not ctx.channels(0)[R].any()
    full = descriptor(v, 1, extraction.ExtractionOptions(channels=ch, variance=True, optimal=True))[1].extraction_plan
    mid = (full.row_windows[:, 0] + full.row_windows[:, 1]) // 2
    short = [(int(m) - lo, int(m) + hi) for m, (lo, hi) in zip(mid, [(1, 2), (0, 1), (3, 4), (2, 3)])]      # 3, 1, 7 and 5 rows
    for run, got, got_var, want in both_sources(
            lambda o: extraction.Extraction(short, channels=ch, row_solution=full.row_solution, variance=extraction.Variances(RN), optimal=o),
            "windows shorter than 8 rows"):
        assert fpl.heights(run.plan.row_windows) == (3, 1, 7, 5) and (got_var > 0.0).all()
    # the binding's bookkeeping: delivering the planes as well does not hide the optimal channels
    ctx.deliver_profile(0)
    assert ctx.has_optimal_channels(0) and ctx.delivers_profile(0)
    ctx.run(0)
    ctx.download_spectra(0)
    assert ctx.optimal_channels(0)[0].tobytes() == got.tobytes() and ctx.profile_planes(0).any()


# ---- the spectra block: one layout, whichever way the options were set (plan::spectra_layout) ----

PRODUCTS = ("spectra", "sky", "n_rejected", "channels", "spectra_var", "sky_var", "channels_var", "optimal", "optimal_var",
            "channels_opt", "channels_opt_var")


def every_product(ctx, slot, spectra, sky):
    sv, kv, cv = ctx.variances(slot)
    op, ov = ctx.optimal(slot)
    co, cov = ctx.optimal_channels(slot)
    return dict(zip(PRODUCTS, (spectra.copy(), sky.copy(), ctx.rejected(slot), ctx.channels(slot), sv, kv, cv, op, ov, co, cov)))


def pinned_addresses(ctx, slot, spectra, sky):
    """{product: address} in the slot's pinned copy: wait_spectra's views and what the accessors return behind it."""
    L, h = ctx._L, ctx._h
    p = {name: (C.POINTER(C.c_uint32)() if name == "n_rejected" else _lib._dp()) for name in PRODUCTS[2:]}
    ref = {name: C.byref(ptr) for name, ptr in p.items()}
    at = {"spectra": spectra.ctypes.data, "sky": sky.ctypes.data}
    assert L.wayne_exposure_rejected(h, slot, ref["n_rejected"]) == 0
    assert L.wayne_exposure_channels(h, slot, ref["channels"]) == 0
    assert L.wayne_exposure_variances(h, slot, ref["spectra_var"], ref["sky_var"], ref["channels_var"]) == 0
    assert L.wayne_exposure_optimal(h, slot, ref["optimal"], ref["optimal_var"]) == 0
    assert L.wayne_exposure_optimal_channels(h, slot, ref["channels_opt"], ref["channels_opt_var"]) == 0
    at.update({name: C.cast(ptr, C.c_void_p).value or 0 for name, ptr in p.items()})
    return at


def test_every_product_lies_where_the_layout_says():
    """tiny_g102: S = 74, R = 2 -- three 4-byte counts, so the channels behind them need padding.  Slot 0 gets every
    option with its upload; slot 1 is uploaded plain and gets them through the context, the variances first and the
    rejection last, switched off and on again.  Same bytes in every product, by either way of fetching, and in the pinned
    copy every product where tests/spectra_layout_law.py puts it."""
    v = visit("tiny_g102")
    ctx = engine_of(v).ctx
    S, R = planes_of(v).S, v.NSAMP - 1
    assert (S, R) == (74, 2)
    ch = extraction.Channels.linear(*WIDE[v.grism.name], 5)
    over = dict(cosmic_rate=busy_rate(v), stellar_flux=np.asarray(v.stellar_flux) * BRIGHTER["tiny_g102"])
    opts = extraction.ExtractionOptions(margin=40, crrej=True, channels=ch, variance=extraction.Variances(RN),
                                        optimal=extraction.Optimal(1, channels=True))
    desc, gen = descriptor(v, 0, opts, **over)
    plan = gen.extraction_plan
    plain, _ = descriptor(v, 0, extraction.ExtractionOptions(margin=40), **over)
    ctx.upload(0, desc)
    ctx.upload(1, plain)
    ctx.set_variance(1, plan.variance)
    ctx.set_optimal(1, extraction.Optimal(1))
    ctx.set_channels(1, plan.channels, plan.row_solution)
    ctx.set_crrej(1, plan.crrej)
    ctx.set_optimal_channels(1)
    ctx.set_crrej(1, None)
    ctx.set_crrej(1, plan.crrej)
    for slot in (0, 1):
        assert ctx.has_crrej(slot) and ctx.has_channels(slot) and ctx.has_variance(slot) and ctx.has_optimal(slot) and ctx.has_optimal_channels(slot)
        ctx.run(slot)
    down = [every_product(ctx, slot, *ctx.download_spectra(slot)) for slot in (0, 1)]
    want, total = sll.layout(S, R, crrej=True, C=5, variance=True, optimal=True, optimal_channels=True)
    assert want["channels"] == want["n_rejected"] + 3 * 4 + 4 and sorted(want) == sorted(PRODUCTS)
    for slot in (0, 1):
        ctx.fetch_spectra_async(slot)
        spectra, sky = ctx.wait_spectra(slot)
        at = pinned_addresses(ctx, slot, spectra, sky)
        assert {name: at[name] - at["spectra"] for name in PRODUCTS} == want, slot
        pinned = every_product(ctx, slot, spectra, sky)
        for name in PRODUCTS:
            assert pinned[name].tobytes() == down[slot][name].tobytes() == down[0][name].tobytes(), (slot, name)
    got = down[0]
    assert got["n_rejected"].sum() > 0 and got["n_rejected"].dtype == np.uint32
    assert all(got[name].any() for name in PRODUCTS) and got["channels_opt"].shape == (R + 1, 5)
