"""GPU: the optimal (profile-weighted) extraction (wayne_exposure_set_optimal; k_extract_optimal and
k_extract_optimal_finish).

The oracle in every parity case is the law restated in numpy (tests/optimal_law.py) applied to the reads of the SAME slot
and to the box arrays the SAME slot delivered (spectra, sky, spectra_var, sky_var: verified against their own laws in
tests/test_extraction_gpu.py, test_crrej_gpu.py and test_variance_gpu.py): only the order of the row sums differs, 2e-9 of
M_U / W on the flux and 4e-9 on the variance (derived in tests/optimal_law.py), and a column that falls back is the box
value to the bit.  Host side, and the same ensemble on CPU-oracle reads: tests/test_optimal.py."""
import collections
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import crrej_law
import extraction_law as law
import helpers
import optimal_law
from wayne_amd import _lib, engine, extraction, run_visit
from wayne_amd.visit import VisitRunner

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MINI = os.path.join(HERE, "fixtures", "mini_visit")
_visits, _planes = {}, {}
Run = collections.namedtuple("Run", "reads spectra sky rejected spectra_var sky_var channels optimal optimal_var plan")
RN = 20.0
HALF_WIDTHS = (1, 8, 16)


def visit(name, n=6):
    if (name, n) not in _visits:
        _visits[(name, n)] = helpers.make_visit(name, n_exposures=n)
    return _visits[(name, n)]


def planes(v):
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
    sv, kv, _ = ctx.variances(slot) if ctx.has_variance(slot) else (None, None, None)
    op, ov = ctx.optimal(slot) if ctx.has_optimal(slot) else (None, None)
    return Run(r, spectra, sky, ctx.rejected(slot) if ctx.has_crrej(slot) else None, sv, kv,
               ctx.channels(slot) if ctx.has_channels(slot) else None, op, ov, plan)


def extracted(v, i, ex, out_dtype=np.float32, slot=0, **over):
    ctx = engine_of(v).ctx
    desc, gen = descriptor(v, i, ex, out_dtype, **over)
    ctx.upload(slot, desc)
    ctx.run(slot)
    return fetch(ctx, slot, gen.extraction_plan)


def oracle_of(run, v, H=None, reads=None):
    plan = run.plan
    cr = (plan.crrej.k, plan.crrej.read_noise) if plan.crrej is not None else None
    return optimal_law.restate(run.reads if reads is None else reads, planes(v), plan.row_windows,
                               plan.optimal.half_width if H is None else H, plan.variance.read_noise, run.spectra, run.sky,
                               run.spectra_var, run.sky_var, plan.steps, cr)


def assert_is_the_law(run, v, what, H=None, reads=None, both=True):
    R, S = v.NSAMP - 1, planes(v).S
    for a in (run.optimal, run.optimal_var):
        assert a.shape == (R + 1, S) and a.dtype == np.float64, what
    want = oracle_of(run, v, H, reads)
    optimal_law.assert_parity(run.optimal, run.optimal_var, want, run.spectra, run.spectra_var, what)
    if both:                                                          # both branches of the law are exercised
        assert want.ok.any() and (~want.ok[:R]).any(), what
    return want


def busy_rate(v, per_interval=30.0):
    dt = np.diff(np.concatenate([[0.0], np.asarray(v.read_times, dtype=float)]))
    N = v.detector.light_sensitive_size(v.SUBARRAY)
    return per_interval * 1024.0 ** 2 / (N * N * dt.min())


def with_every_half_width(v, i, ex, out_dtype, what, **over):
    """One upload; a run and a comparison per half width (a second run of a slot synthesises the same reads); at every
    half width both branches of the law must be exercised: some column takes the optimal values, some the box's."""
    ctx = engine_of(v).ctx
    desc, gen = descriptor(v, i, ex, out_dtype, **over)
    ctx.upload(0, desc)
    plan = gen.extraction_plan
    reads, runs = None, []
    for H in HALF_WIDTHS:
        ctx.set_optimal(0, extraction.Optimal(H))
        ctx.run(0)
        run = fetch(ctx, 0, plan, reads=reads is None)
        reads = run.reads if reads is None else reads
        if plan.crrej is not None and not runs:
            # the numpy law must decide every flag as the device did, or a pixel's v is another number
            cr = plan.crrej
            mask = crrej_law.restate(reads, planes(v), plan.row_windows, plan.bg_cols, plan.steps, cr.k, cr.read_noise).mask
            assert (ctx.download_crmask(0) == mask).all(), what
            assert run.rejected.sum() > 0, what
        assert_is_the_law(run, v, "%s H %d" % (what, H), H, reads)
        runs.append(run)
    # the box extraction does not see the half width; the optimal one does
    for run in runs[1:]:
        assert run.spectra.tobytes() == runs[0].spectra.tobytes() and run.spectra_var.tobytes() == runs[0].spectra_var.tobytes()
        assert run.optimal.tobytes() != runs[0].optimal.tobytes()
    return runs


VISITS = [("tiny", 0), ("tiny_g102", 0), ("tiny128", 0), ("small256", 1), ("stare256", 0)]
# The star of the three small visits is too faint for ok(x): their brightest column holds some 450 e- against 160 e- of
# read noise in a 64-row window, and on CPU-oracle reads not one column of `tiny` passes the 3 sigma test at H = 1, 8 or 16
# (tiny_g102: 0, 1 and 10 columns; tiny128: 1, 3 and 2) -- the optimal branch would never run on the frames that have the
# partial tile and the left clamp.  So their star is 30 times brighter here (25 to 59 columns then pass in every product
# and at every half width, the others fall back); frame, tiles, windows and clamps are the visit's own.
BRIGHTER = {"tiny": 30.0, "tiny_g102": 30.0, "tiny128": 30.0}


@pytest.mark.parametrize("crrej", [False, True], ids=["plain", "crrej"])
@pytest.mark.parametrize("out_dtype", [np.float32, np.float64, np.uint16], ids=["f32", "f64", "u16"])
@pytest.mark.parametrize("name,i", VISITS, ids=[n for n, _ in VISITS])
def test_optimal_is_the_law_applied_to_the_slots_reads_and_box_arrays(name, i, out_dtype, crrej):
    v = visit(name)
    margin = 40 if name in ("tiny", "tiny_g102") else extraction.ROW_MARGIN
    ex = extraction.ExtractionOptions(margin=margin, crrej=crrej or None, variance=extraction.Variances(RN), optimal=True)
    # (the siblings' rates: tests/test_crrej_gpu.py for the 64-pixel frames, tests/test_variance_gpu.py for the others)
    over = dict(cosmic_rate=busy_rate(v) if name.startswith("tiny") else busy_rate(v, 3.0)) if crrej else {}
    if name in BRIGHTER:
        over["stellar_flux"] = np.asarray(v.stellar_flux) * BRIGHTER[name]
    what = "%s[%d] %s crrej %d" % (name, i, np.dtype(out_dtype).name, crrej)
    runs = with_every_half_width(v, i, ex, out_dtype, what, **over)
    S = planes(v).S
    if name in ("tiny", "tiny_g102"):
        assert S == 74                                                 # a partial last tile; X(x) is clamped on the left in tile 0
    if name == "small256":
        R = v.NSAMP - 1
        rows = runs[0].plan.row_windows[R, 1] - runs[0].plan.row_windows[R, 0]
        assert rows > 2 * 32 and rows % 32 != 0                        # several chunks and a remainder


def test_steps_off_and_short_windows():
    v = visit("small256")
    R, S = v.NSAMP - 1, planes(v).S
    for steps in (extraction.ALL & ~extraction.SKY, extraction.ALL & ~extraction.LAST_READ):
        run = extracted(v, 1, extraction.ExtractionOptions(steps=steps, variance=True, optimal=True))
        assert_is_the_law(run, v, "steps %d" % steps)
        if not steps & extraction.LAST_READ:
            assert not run.optimal[R].any() and not run.optimal_var[R].any() and run.optimal[:R].any()
        if not steps & extraction.SKY:
            assert (run.sky == 0.0).all() and (run.sky_var == 0.0).all()
    # windows shorter than the 8 waves of a workgroup, about the middle of the default plan's (where the star crosses)
    full = extracted(v, 1, extraction.ExtractionOptions(variance=True, optimal=True)).plan
    mid = (full.row_windows[:, 0] + full.row_windows[:, 1]) // 2
    short = [(int(m) - lo, int(m) + hi) for m, (lo, hi) in zip(mid, [(1, 2), (0, 1), (3, 4), (2, 3)])]      # 3, 1, 7 and 5 rows
    run = extracted(v, 1, extraction.Extraction(short, variance=extraction.Variances(RN), optimal=extraction.Optimal(8)))
    assert_is_the_law(run, v, "windows shorter than 8 rows")


def test_the_same_exposure_gives_the_same_bytes():
    v = visit("small256")
    ctx = engine_of(v).ctx
    desc, gen = descriptor(v, 1, extraction.ExtractionOptions(crrej=True, variance=True, optimal=True),
                           cosmic_rate=busy_rate(v, 3.0))
    plan = gen.extraction_plan
    for slot in (0, 1):                                              # the two streams
        ctx.upload(slot, desc)
        ctx.run(slot)
    a, b = fetch(ctx, 0, plan), fetch(ctx, 1, plan)
    for name in ("optimal", "optimal_var", "spectra", "spectra_var"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert a.optimal.max() > 1e4 and a.optimal.tobytes() != a.spectra.tobytes()
    for slot, i in ((0, 0), (1, 2)):                                 # other exposures, with other plans, in between
        other, _ = descriptor(v, i, extraction.ExtractionOptions(margin=3 + slot, variance=extraction.Variances(5.0 + slot),
                                                                 optimal=extraction.Optimal(3 + slot)))
        ctx.upload(slot, other)
        ctx.run(slot)
    ctx.synchronize()
    ctx.upload(3, desc)
    ctx.run(3)
    c = fetch(ctx, 3, plan)
    ctx.run(3)                                                       # a second run sums again, it does not add
    d = fetch(ctx, 3, plan)
    for name in ("optimal", "optimal_var"):
        assert getattr(c, name).tobytes() == getattr(a, name).tobytes() == getattr(d, name).tobytes(), name
    # the delivery path (pinned copy) brings the same bytes
    ctx.fetch_spectra_async(3)
    spectra, _ = ctx.wait_spectra(3)
    op, ov = ctx.optimal(3)
    assert op.tobytes() == a.optimal.tobytes() and ov.tobytes() == a.optimal_var.tobytes()
    assert spectra.tobytes() == a.spectra.tobytes() and ctx.variances(3)[0].tobytes() == a.spectra_var.tobytes()


def pinned_block(ctx, slot, n_bytes):
    """(the first `n_bytes` of the slot's pinned spectra block, rc of wayne_exposure_optimal, the addresses of spectra,
    optimal and optimal_var in it; 0: a null pointer)."""
    ctx.fetch_spectra_async(slot)
    ps, pk = _lib._dp(), _lib._dp()
    assert ctx._L.wayne_exposure_wait_spectra(ctx._h, slot, C.byref(ps), C.byref(pk)) == 0
    po, pv = _lib._dp(), _lib._dp()
    rc = ctx._L.wayne_exposure_optimal(ctx._h, slot, C.byref(po), C.byref(pv))
    addr = [C.cast(p, C.c_void_p).value or 0 for p in (ps, po, pv)]
    return C.string_at(addr[0], n_bytes), rc, addr


def test_off_means_off():
    v = visit("small256")
    ctx = engine_of(v).ctx
    R, S = v.NSAMP - 1, planes(v).S
    over = dict(cosmic_rate=busy_rate(v, 3.0))
    ch = extraction.Channels.linear(1.05, 1.75, 23)
    for crrej in (None, True):
        for channels in (None, ch):
            on, gen = descriptor(v, 1, extraction.ExtractionOptions(crrej=crrej, channels=channels, variance=True, optimal=True), **over)
            plan = gen.extraction_plan
            # the block without the option: its length, which nothing here writes down twice, is what lies in front of
            # optimal once the option is on
            block = (R + 1) * (S + 1) * 8 + ((R + 1) * 4 if crrej else 0)
            block = (block + 7) // 8 * 8 + ((R + 1) * ch.n * 8 if channels else 0)
            block += (R + 1) * (S + 1 + (ch.n if channels else 0)) * 8
            ctx.upload(0, on)
            ctx.set_optimal(0, None)                                 # the same exposure, before set_optimal
            assert not ctx.has_optimal(0) and ctx.has_variance(0)
            ctx.run(0)
            never = fetch(ctx, 0, plan.with_optimal(None))
            assert never.optimal is None
            with pytest.raises(_lib.WayneError) as e:
                ctx.optimal(0)
            assert e.value.status == _lib.E_STATE
            before, rc, _ = pinned_block(ctx, 0, block)
            assert rc == _lib.E_STATE
            ctx.set_optimal(0, True)
            assert ctx.has_optimal(0) and ctx.has_variance(0) and ctx.has_crrej(0) == bool(crrej)
            ctx.run(0)
            got = fetch(ctx, 0, plan)
            for name in ("reads", "spectra", "sky", "spectra_var", "sky_var") + (("channels",) if channels else ()) + (("rejected",) if crrej else ()):
                assert getattr(got, name).tobytes() == getattr(never, name).tobytes(), name
            assert ctx.variances(0)[2] is None or ctx.variances(0)[2].tobytes() == before[-(R + 1) * ch.n * 8:]
            # the pinned copy: everything that was there lies where it lay, byte for byte, and optimal begins where it ended
            after, rc, (sp, po, pv) = pinned_block(ctx, 0, block)
            assert rc == 0 and after == before
            assert po - sp == block and pv - po == (R + 1) * S * 8
            op, ov = ctx.optimal(0)
            assert op.tobytes() == got.optimal.tobytes() and ov.tobytes() == got.optimal_var.tobytes()
            assert op.tobytes() == C.string_at(po, (R + 1) * S * 8)
            # set_crrej and set_channels keep it (the layout follows them); None, set_variance, a fresh upload and
            # set_extraction clear it
            ctx.set_crrej(0, extraction.CosmicRejection() if crrej else None)
            assert ctx.has_optimal(0)
            ctx.run(0)
            assert fetch(ctx, 0, plan, reads=False).optimal.tobytes() == got.optimal.tobytes()
            ctx.set_optimal(0, None)
            ctx.upload(1, on)
            ctx.set_variance(1, True)
            ctx.upload(2, on)
            ctx.set_extraction(2, plan.with_optimal(None))
            for slot in (0, 1, 2):
                assert not ctx.has_optimal(slot) and ctx.has_variance(slot)
                ctx.run(slot)
                again = fetch(ctx, slot, plan.with_optimal(None), reads=False)
                assert again.optimal is None and again.spectra.tobytes() == never.spectra.tobytes()
                assert again.spectra_var.tobytes() == never.spectra_var.tobytes()
                po, pv = _lib._dp(), _lib._dp()
                assert ctx._L.wayne_exposure_optimal(ctx._h, slot, C.byref(po), C.byref(pv)) == _lib.E_STATE
                assert pinned_block(ctx, slot, block)[0] == before


def test_refusals_leave_the_slot_extracting_with_variances():
    v = visit("small256")
    ctx = engine_of(v).ctx
    plain, gen = descriptor(v, 1, True)
    ctx.upload(0, plain)
    with pytest.raises(_lib.WayneError) as e:                        # no variances on the slot
        ctx.set_optimal(0, True)
    assert e.value.status == _lib.E_STATE and not ctx.has_optimal(0)
    nothing, _ = descriptor(v, 1, None)
    ctx.upload(0, nothing)
    with pytest.raises(_lib.WayneError) as e:                        # no extraction either
        ctx.set_optimal(0, True)
    assert e.value.status == _lib.E_STATE
    with_var, gen = descriptor(v, 1, extraction.ExtractionOptions(variance=True))
    ctx.upload(1, with_var)
    ctx.run(1)
    never = fetch(ctx, 1, gen.extraction_plan, reads=False)

    def raw(slot, H):
        d = _lib.OptimalDesc(H)
        return ctx._L.wayne_exposure_set_optimal(ctx._h, slot, C.byref(d))

    for H in (0, 17, -1, 2 ** 31 - 1, -2 ** 31):
        ctx.upload(0, with_var)
        ctx.set_optimal(0, True)
        assert raw(0, H) == _lib.E_INVALID, H
    ctx.run(0)                                                       # ... and the slot extracts, with variances, without optimal
    got_spectra, _ = ctx.download_spectra(0)
    assert got_spectra.tobytes() == never.spectra.tobytes() and ctx.variances(0)[0].tobytes() == never.spectra_var.tobytes()
    po, pv = _lib._dp(), _lib._dp()
    assert ctx._L.wayne_exposure_optimal(ctx._h, 0, C.byref(po), C.byref(pv)) == _lib.E_STATE
    # the optimal values exist once the spectra have been fetched
    for H in (1, 16):
        assert raw(0, H) == 0
    ctx.set_optimal(0, 8)
    ctx.run(0)
    with pytest.raises(_lib.WayneError) as e:
        ctx.optimal(0)
    assert e.value.status == _lib.E_STATE
    ctx.download_spectra(0)
    op, ov = ctx.optimal(0)
    assert op.shape == ov.shape == (v.NSAMP, 266)


class SameExposure(VisitRunner):
    """Every index is exposure 0 of the visit with the index's own random draws: no cosmic rays, no scan-speed variation,
    no flat (the set-up of tests/test_variance_gpu.py's ensemble)."""

    def frame_kwargs(self, i):
        return self.visit.frame_kwargs(0, cosmic_rate=None, ssv_generator=None, add_flat=False)


def test_the_optimal_extraction_beats_the_box_on_the_devices_reads():
    """The ensemble of tests/test_optimal.py on device reads: 32 exposures of small256 that differ in their random draws
    alone, through VisitRunner, H = 8, sums over columns 59 .. 188 of the last-read product.  The bounds are those of the
    CPU test, derived there: variance ratio <= 0.8, |paired bias| <= 1e-3, ensemble / predicted variance within
    1 +- 4 sqrt(2 / (130 x 31)) = 1 +- 0.089.  The read intervals' figures are printed, not asserted (interval 0 is the
    stated limit: the profile's own noise is not in 1 / W)."""
    v = visit("small256")
    n, cols = 32, (59, 189)
    runner = SameExposure(v)
    spectra, _ = runner.run_spectra(range(n), extraction=extraction.ExtractionOptions(variance=extraction.Variances(RN),
                                                                                      optimal=extraction.Optimal(8)))
    R = v.NSAMP - 1
    assert runner.optimal.shape == runner.optimal_var.shape == spectra.shape == (n, R + 1, planes(v).S)
    assert spectra[0].tobytes() != spectra[1].tobytes()
    sd = np.sqrt(2.0 / ((cols[1] - cols[0]) * (n - 1)))
    for p in list(range(R)) + [R]:
        ratio, bias, predicted = optimal_law.ensemble_figures(runner.optimal[:, p], runner.optimal_var[:, p], spectra[:, p], cols)
        print("device, %d exposures, %s: ensemble variance box %.4g, optimal / box %.3f; bias %+.2e; ensemble / predicted "
              "variance %.3f" % (n, "last read" if p == R else "interval %d" % p,
                                 spectra[:, p, cols[0]:cols[1]].var(axis=0, ddof=1).sum(), ratio, bias, predicted))
    assert (spectra[:, R, cols[0]:cols[1]].mean(axis=0) > 1e3).all()   # the columns do lie on the trace
    assert ratio <= 0.8
    assert abs(bias) <= 1e-3
    assert abs(predicted - 1.0) <= 4 * sd


def test_frames_visits_and_observations_carry_the_optimal_extraction(tmp_path):
    v = visit("tiny")
    exp = helpers.product_generator(v, 0).scanning_frame(extraction=True, variance=True, optimal=True, **v.frame_kwargs(0))
    assert exp.optimal.shape == exp.optimal_var.shape == (4, 74) and exp.extraction.optimal.half_width == 8
    plain = helpers.product_generator(v, 0).scanning_frame(extraction=True, variance=True, **v.frame_kwargs(0))
    assert not hasattr(plain, "optimal") and plain.spectra.tobytes() == exp.spectra.tobytes()
    assert plain.spectra_var.tobytes() == exp.spectra_var.tobytes()
    run = Run(np.stack([r[0] for r in exp.reads]), exp.spectra, exp.sky, None, exp.spectra_var, exp.sky_var, None, exp.optimal,
              exp.optimal_var, exp.extraction)
    assert_is_the_law(run, v, "scanning_frame(optimal=True)", both=False)
    with pytest.raises(ValueError):
        helpers.product_generator(v, 0).scanning_frame(extraction=True, optimal=True, **v.frame_kwargs(0))

    runner = VisitRunner(v)
    opts = extraction.ExtractionOptions(variance=True, optimal=True)
    runner.run_spectra(range(3), extraction=opts)
    assert runner.optimal.shape == runner.optimal_var.shape == (3, 4, 74)
    assert runner.optimal[0].tobytes() == exp.optimal.tobytes() and runner.optimal_var[0].tobytes() == exp.optimal_var.tobytes()
    runner.run_spectra(range(2), extraction=extraction.ExtractionOptions(variance=True))
    assert runner.optimal is None and runner.optimal_var is None and runner.spectra_var is not None
    runner.run(range(2), extraction=opts)
    assert sorted(runner.optimal) == [0, 1] and runner.optimal[0].tobytes() == exp.optimal.tobytes()
    assert runner.optimal_var[0].tobytes() == exp.optimal_var.tobytes()
    runner.run(range(1), extraction=True)
    assert runner.optimal is None

    s = visit("stare256")
    kw = s.frame_kwargs(0)
    for drop in ("scan_speed", "sample_rate", "ssv_generator"):
        kw.pop(drop, None)
    stare = helpers.product_generator(s, 0).staring_frame(extraction=True, variance=True, optimal=extraction.Optimal(4), **kw)
    assert stare.optimal.shape == (4, 266) and stare.optimal.max() > 1e4 and stare.extraction.optimal.half_width == 4

    # the CLI: --optimal writes the frames' own arrays
    work = str(tmp_path / "visit")
    shutil.copytree(MINI, work)
    yml = os.path.join(work, "params.yml")
    out, plain_npz = str(tmp_path / "opt.npz"), str(tmp_path / "plain.npz")
    base = ["spectra", "sky", "exposure_index", "row_lo", "row_hi", "bg_cols", "x_ref", "y_ref", "read_times", "exp_start",
            "spectra_var", "sky_var", "variance_read_noise"]
    obs = run_visit.run(["-p", yml, "--max-exposures", "3", "--spectra-only", out, "--variances", "--optimal", "5"])
    z = np.load(out)
    assert sorted(z.files) == sorted(base + ["optimal", "optimal_var", "optimal_half_width"])
    assert z["optimal"].shape == z["optimal_var"].shape == z["spectra"].shape and int(z["optimal_half_width"]) == 5
    np.testing.assert_array_equal(z["optimal"], obs.spectra_result["optimal"])
    obs2 = run_visit.run(["-p", yml, "--max-exposures", "3", "--spectra-only", plain_npz, "--variances"])
    zp = np.load(plain_npz)
    assert sorted(zp.files) == sorted(base) and "optimal" not in obs2.spectra_result
    assert zp["spectra"].tobytes() == z["spectra"].tobytes() and zp["spectra_var"].tobytes() == z["spectra_var"].tobytes()
    # Observation.frame_options["optimal"] through the frame API: the same exposure, the same bytes
    obs2.frame_options["optimal"] = extraction.Optimal(5)
    obs2.spectra_out, obs2.spectra_only = None, False
    frame = obs2._generate_exposure(obs2.exp_start_times[1], 2, write_fits=False)
    assert frame.optimal.tobytes() == z["optimal"][1].tobytes() and frame.optimal_var.tobytes() == z["optimal_var"][1].tobytes()
