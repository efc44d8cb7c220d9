"""GPU: variances of the device-side extraction (wayne_exposure_set_variance; the VAR instantiations of k_extract_rows,
k_extract_finish, k_extract_bins and k_extract_bins_finish).

The oracle in every parity case is the law restated in numpy (tests/variance_law.py) applied to the reads of the SAME
slot: a variance may differ from it by the order of its float64 sums alone, 1e-9 of the variance itself (derived in
tests/variance_law.py).  Host side, and the same ensemble on CPU-oracle reads: tests/test_variance.py."""
import collections
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import channel_law
import crrej_law
import extraction_law as law
import helpers
import variance_law
from wayne_amd import _lib, engine, extraction, run_visit
from wayne_amd.visit import VisitRunner

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MINI = os.path.join(HERE, "fixtures", "mini_visit")
_visits, _planes, _flats = {}, {}, {}
Run = collections.namedtuple("Run", "reads spectra sky channels rejected spectra_var sky_var channels_var plan")
WIDE = {"G141": (1.0, 1.8), "G102": (0.7, 1.25)}          # beyond the first order at both ends
RN = 20.0


def visit(name, n=6):
    if (name, n) not in _visits:
        _visits[(name, n)] = helpers.make_visit(name, n_exposures=n)
    return _visits[(name, n)]


def planes(v):
    if v.name not in _planes:
        _planes[v.name] = law.Planes(v)
    return _planes[v.name]


def flat_of(v):
    if v.name not in _flats:
        _flats[v.name] = channel_law.Flat(v)
    return _flats[v.name]


def engine_of(v):
    return engine.get_engine(0, v.grism, v.detector, v.calibration, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)


def descriptor(v, i, ex, out_dtype=np.float32, **over):
    gen = helpers.product_generator(v, i)
    return gen.build_descriptor(engine_of(v), out_dtype=out_dtype, extraction=ex, **v.frame_kwargs(i, **over)), gen


def fetch(ctx, slot, plan, reads=True):
    r = ctx.download(slot) if reads else None
    spectra, sky = ctx.download_spectra(slot)
    sv, kv, cv = ctx.variances(slot) if ctx.has_variance(slot) else (None, None, None)
    return Run(r, spectra, sky, ctx.channels(slot) if ctx.has_channels(slot) else None,
               ctx.rejected(slot) if ctx.has_crrej(slot) else None, sv, kv, cv, plan)


def extracted(v, i, ex, out_dtype=np.float32, slot=0, **over):
    ctx = engine_of(v).ctx
    desc, gen = descriptor(v, i, ex, out_dtype, **over)
    ctx.upload(slot, desc)
    ctx.run(slot)
    return fetch(ctx, slot, gen.extraction_plan)


def oracle_of(run, v):
    plan = run.plan
    cr = (plan.crrej.k, plan.crrej.read_noise) if plan.crrej is not None else None
    ch = {}
    if plan.channels is not None:
        ch = dict(edges=plan.channels.edges_um, wl_a=plan.row_solution[0], wl_b=plan.row_solution[1],
                  flat=flat_of(v) if plan.channels.flat else None)
    return variance_law.restate(run.reads, planes(v), plan.row_windows, plan.bg_cols, plan.variance.read_noise, plan.steps,
                                cr, **ch)


def assert_is_the_law(run, v, what):
    R, S = v.NSAMP - 1, planes(v).S
    assert run.spectra_var.shape == (R + 1, S) and run.spectra_var.dtype == np.float64
    assert run.sky_var.shape == (R + 1,) and run.sky_var.dtype == np.float64
    if run.plan.crrej is not None:
        # (a flag the device may decide the other way changes a pixel's v: the exposure must have none)
        cr = run.plan.crrej
        assert not crrej_law.restate(run.reads, planes(v), run.plan.row_windows, run.plan.bg_cols, run.plan.steps, cr.k,
                                     cr.read_noise).undecided.any(), what
    want = oracle_of(run, v)
    variance_law.assert_parity(run.spectra_var, run.sky_var, run.channels_var, want, what)
    return want


def busy_rate(v, per_interval=30.0):
    dt = np.diff(np.concatenate([[0.0], np.asarray(v.read_times, dtype=float)]))
    N = v.detector.light_sensitive_size(v.SUBARRAY)
    return per_interval * 1024.0 ** 2 / (N * N * dt.min())


def parity_case(name, i, out_dtype, flat, crrej=False, n_channels=20):
    v = visit(name)
    lo, hi = WIDE[v.grism.name]
    ch = extraction.Channels.linear(lo, hi, n_channels).with_flat(flat)
    margin = 40 if name.startswith("tiny") and name != "tiny128" else extraction.ROW_MARGIN
    ex = extraction.ExtractionOptions(margin=margin, channels=ch, crrej=crrej or None, variance=extraction.Variances(RN))
    over = dict(cosmic_rate=busy_rate(v, 3.0)) if crrej else {}
    run = extracted(v, i, ex, out_dtype, **over)
    R, S = v.NSAMP - 1, planes(v).S
    what = "%s[%d] %s flat %d crrej %d" % (name, i, np.dtype(out_dtype).name, flat, crrej)
    assert run.channels_var.shape == (R + 1, n_channels) and run.channels_var.dtype == np.float64
    if name in ("tiny", "tiny_g102"):
        assert S == 74                                                 # the last 64-column tile is partial
    if name == "small256":
        rows = run.plan.row_windows[R, 1] - run.plan.row_windows[R, 0]
        assert rows > 2 * 32 and rows % 32 != 0                        # several chunks and a remainder
    if crrej:
        assert run.rejected.sum() > 0
    want = assert_is_the_law(run, v, what)
    # the read noise of every pixel of a window is in it, and the trace's photons on top
    rows = run.plan.row_windows[:, 1] - run.plan.row_windows[:, 0]
    assert (run.spectra_var >= 0.99 * RN * RN * rows[:, None] * 0.5).all()
    assert (run.sky_var > 0.0).all() and (run.channels_var >= 0.0).all() and run.channels_var.max() > 0.0
    if crrej:
        plain = variance_law.restate(run.reads, planes(v), run.plan.row_windows, run.plan.bg_cols, RN, run.plan.steps, None,
                                     edges=ch.edges_um, wl_a=run.plan.row_solution[0], wl_b=run.plan.row_solution[1],
                                     flat=flat_of(v) if flat else None)
        assert np.abs(plain.spectra_var - want.spectra_var).max() > 1000.0      # the rejection matters to the variances
    return run, want


@pytest.mark.parametrize("flat", [True, False], ids=["flat", "noflat"])
@pytest.mark.parametrize("out_dtype", [np.float32, np.float64, np.uint16], ids=["f32", "f64", "u16"])
@pytest.mark.parametrize("name,i", [("tiny", 0), ("tiny_g102", 0), ("tiny128", 0), ("small256", 1), ("stare256", 0)],
                         ids=["tiny", "tiny_g102", "tiny128", "small256", "stare256"])
def test_variances_are_the_law_applied_to_the_slots_reads(name, i, out_dtype, flat):
    parity_case(name, i, out_dtype, flat)


@pytest.mark.parametrize("flat", [True, False], ids=["flat", "noflat"])
@pytest.mark.parametrize("out_dtype", [np.float32, np.float64, np.uint16], ids=["f32", "f64", "u16"])
def test_variances_of_a_rejecting_extraction_are_the_law(out_dtype, flat):
    parity_case("small256", 1, out_dtype, flat, crrej=True)


@pytest.mark.parametrize("crrej", [None, True], ids=["plain", "crrej"])
def test_variances_without_channels(crrej):
    v = visit("small256")
    over = dict(cosmic_rate=busy_rate(v, 3.0)) if crrej else {}
    run = extracted(v, 1, extraction.ExtractionOptions(crrej=crrej, variance=True), **over)
    assert run.channels_var is None and run.channels is None and run.plan.variance.read_noise == 20.0
    assert_is_the_law(run, v, "no channels, crrej %s" % bool(crrej))


def test_steps_off():
    v = visit("small256")
    ch = extraction.Channels.linear(1.1, 1.7, 20)
    for steps in (extraction.ALL & ~extraction.LAST_READ, extraction.ALL & ~extraction.SKY, extraction.GAIN):
        run = extracted(v, 1, extraction.ExtractionOptions(steps=steps, channels=ch, variance=True))
        assert_is_the_law(run, v, "steps %d" % steps)
        if not steps & extraction.LAST_READ:
            assert not run.spectra_var[-1].any() and not run.channels_var[-1].any() and run.sky_var[-1] == 0.0
            assert run.spectra_var[:-1].all()
        if not steps & extraction.SKY:
            formed = v.NSAMP if steps & extraction.LAST_READ else v.NSAMP - 1
            assert (run.sky_var == 0.0).all() and (run.sky == 0.0).all() and run.spectra_var[:formed].all()


def test_short_and_odd_windows():
    v = visit("small256")
    S = 266
    px = 2.0 ** -7
    sol = (np.full(S, 0.5), np.full(S, px))
    edges = 0.5 + px * np.array([30.0, 31.0, 40.5, 100.0, 180.25, 250.0])
    cases = {
        "not a multiple of 32": [(100, 137), (110, 153), (120, 185), (20, 243)],        # 37, 43, 65 and 223 rows
        "shorter than 8 rows": [(100, 103), (7, 8), (S - 12, S - 5), (130, 135)],       # 3, 1, 7 and 5 rows
    }
    for what, windows in cases.items():
        for ch in (extraction.Channels(edges, flat=True), None):
            plan = extraction.Extraction(windows, channels=ch, row_solution=sol if ch is not None else None,
                                         variance=extraction.Variances(RN))
            run = extracted(v, 0, plan)
            assert_is_the_law(run, v, "%s, channels %s" % (what, ch is not None))


def test_integer_edges_give_the_devices_own_column_variances():
    v = visit("small256")
    S = 266
    px = 2.0 ** -7
    sol = (np.full(S, 0.5), np.full(S, px))
    cols = [30, 31, 40, 100, 180, 250]
    plan = extraction.Extraction([(100, 140), (110, 150), (120, 167), (20, 246)], steps=extraction.ALL & ~extraction.SKY,
                                 channels=extraction.Channels(0.5 + px * np.array(cols, dtype=float), flat=False),
                                 row_solution=sol, variance=True)
    run = extracted(v, 0, plan)
    assert_is_the_law(run, v, "integer edges, sky off")
    for b in range(5):
        col = run.spectra_var[:, cols[b]:cols[b + 1]].sum(axis=1)
        assert (np.abs(run.channels_var[:, b] - col) <= law.REL * col).all(), b


def test_the_same_exposure_gives_the_same_bytes():
    v = visit("small256")
    ctx = engine_of(v).ctx
    ch = extraction.Channels.linear(1.05, 1.75, 23)
    desc, gen = descriptor(v, 1, extraction.ExtractionOptions(channels=ch, crrej=True, variance=True),
                           cosmic_rate=busy_rate(v, 3.0))
    for slot in (0, 1):                                              # the two streams
        ctx.upload(slot, desc)
        ctx.run(slot)
    a, b = fetch(ctx, 0, gen.extraction_plan), fetch(ctx, 1, gen.extraction_plan)
    for name in ("spectra_var", "sky_var", "channels_var", "spectra", "channels"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert a.spectra_var.max() > 1e4 and a.channels_var.max() > 1e4
    for slot, i in ((0, 0), (1, 2), (2, 0)):                         # other exposures, with other plans, in between
        other, _ = descriptor(v, i, extraction.ExtractionOptions(margin=3 + slot, channels=extraction.Channels.linear(1.2, 1.6, 5 + slot),
                                                                 variance=extraction.Variances(5.0 + slot)))
        ctx.upload(slot, other)
        ctx.run(slot)
    ctx.synchronize()
    ctx.upload(3, desc)
    ctx.run(3)
    c = fetch(ctx, 3, gen.extraction_plan)
    ctx.run(3)                                                       # a second run sums again, it does not add
    d = fetch(ctx, 3, gen.extraction_plan)
    for name in ("spectra_var", "sky_var", "channels_var"):
        assert getattr(c, name).tobytes() == getattr(a, name).tobytes() == getattr(d, name).tobytes(), name
    # the delivery path (pinned copy) brings the same bytes
    ctx.fetch_spectra_async(3)
    spectra, sky = ctx.wait_spectra(3)
    sv, kv, cv = ctx.variances(3)
    assert sv.tobytes() == a.spectra_var.tobytes() and kv.tobytes() == a.sky_var.tobytes() and cv.tobytes() == a.channels_var.tobytes()
    assert spectra.tobytes() == a.spectra.tobytes() and ctx.channels(3).tobytes() == a.channels.tobytes()


def pinned_layout(ctx, slot):
    """(spectra, sky, spectra_var, sky_var, channels_var) addresses of the slot's pinned copy (0: a null pointer)."""
    ctx.fetch_spectra_async(slot)
    ps, pk = _lib._dp(), _lib._dp()
    assert ctx._L.wayne_exposure_wait_spectra(ctx._h, slot, C.byref(ps), C.byref(pk)) == 0
    vs, vk, vc = _lib._dp(), _lib._dp(), _lib._dp()
    rc = ctx._L.wayne_exposure_variances(ctx._h, slot, C.byref(vs), C.byref(vk), C.byref(vc))
    addr = [C.cast(p, C.c_void_p).value or 0 for p in (ps, pk, vs, vk, vc)]
    return rc, addr


def test_off_means_off():
    v = visit("small256")
    ctx = engine_of(v).ctx
    R, S = v.NSAMP - 1, planes(v).S
    over = dict(cosmic_rate=busy_rate(v, 3.0))
    ch = extraction.Channels.linear(1.05, 1.75, 23)
    for crrej in (None, True):
        for channels in (None, ch):
            off, gen = descriptor(v, 1, extraction.ExtractionOptions(crrej=crrej, channels=channels), **over)
            on, gen_v = descriptor(v, 1, extraction.ExtractionOptions(crrej=crrej, channels=channels, variance=True), **over)
            ctx.upload(0, off)
            ctx.run(0)
            never = fetch(ctx, 0, gen.extraction_plan)
            assert never.spectra_var is None and not ctx.has_variance(0)
            with pytest.raises(_lib.WayneError) as e:
                ctx.variances(0)
            assert e.value.status == _lib.E_STATE
            ctx.upload(1, on)
            assert ctx.has_variance(1) and ctx.has_crrej(1) == bool(crrej) and ctx.has_channels(1) == (channels is not None)
            ctx.run(1)
            got = fetch(ctx, 1, gen_v.extraction_plan)
            for name in ("reads", "spectra", "sky") + (("channels",) if channels else ()) + (("rejected",) if crrej else ()):
                assert getattr(got, name).tobytes() == getattr(never, name).tobytes(), name
            if crrej:
                assert got.rejected.sum() > 0
            # the pinned copy: everything that was there lies where it lay, and the variances begin where it ended --
            # behind sky, the counts (rounded up to 8 bytes) and the channels
            block = (R + 1) * (S + 1) * 8 + ((R + 1) * 4 if crrej else 0)
            block = (block + 7) // 8 * 8 + ((R + 1) * ch.n * 8 if channels else 0)
            rc, (sp, sk, vs, vk, vc) = pinned_layout(ctx, 0)
            assert rc == _lib.E_STATE and (vs, vk, vc) == (0, 0, 0) and sk - sp == (R + 1) * S * 8
            rc, (sp, sk, vs, vk, vc) = pinned_layout(ctx, 1)
            assert rc == 0 and sk - sp == (R + 1) * S * 8
            assert vs - sp == block and vk - vs == (R + 1) * S * 8
            assert vc == (vk + (R + 1) * 8 if channels else 0)
            sv, kv, cv = ctx.variances(1)
            assert sv.tobytes() == got.spectra_var.tobytes() and kv.tobytes() == got.sky_var.tobytes()
            assert (cv is None) == (channels is None) and (cv is None or cv.tobytes() == got.channels_var.tobytes())
            # set_crrej and set_channels keep the variances (the layout follows them); None, a fresh upload and
            # set_extraction clear them
            ctx.set_crrej(1, extraction.CosmicRejection() if crrej else None)
            assert ctx.has_variance(1)
            ctx.run(1)
            assert fetch(ctx, 1, gen_v.extraction_plan).spectra_var.tobytes() == got.spectra_var.tobytes()
            ctx.set_variance(1, None)
            assert not ctx.has_variance(1)
            ctx.upload(2, on)
            ctx.set_extraction(2, gen.extraction_plan)
            assert not ctx.has_variance(2)
            ctx.upload(3, on)
            ctx.upload(3, off)
            for slot in (1, 2, 3):
                ctx.run(slot)
                again = fetch(ctx, slot, gen.extraction_plan)
                assert again.spectra_var is None and again.spectra.tobytes() == never.spectra.tobytes()
                with pytest.raises(_lib.WayneError) as e:
                    ctx.variances(slot)
                assert e.value.status == _lib.E_STATE


def test_set_variance_before_and_after_the_channels():
    v = visit("small256")
    ctx = engine_of(v).ctx
    ch = extraction.Channels.linear(1.05, 1.75, 23)
    desc, gen = descriptor(v, 1, extraction.ExtractionOptions(channels=ch, variance=extraction.Variances(RN)))
    ctx.upload(0, desc)                                              # (set_extraction: channels first, then variances)
    ctx.run(0)
    want = fetch(ctx, 0, gen.extraction_plan)
    plan = gen.extraction_plan
    plain, _ = descriptor(v, 1, plan.with_channels(None).with_variance(None))
    ctx.upload(1, plain)
    ctx.set_variance(1, extraction.Variances(RN))                    # variances first ...
    ctx.run(1)
    alone = fetch(ctx, 1, plan, reads=False)
    assert alone.channels_var is None and alone.spectra_var.tobytes() == want.spectra_var.tobytes()
    ctx.set_channels(1, plan.channels, plan.row_solution)            # ... then the channels: channels_var comes too
    assert ctx.has_variance(1)
    ctx.run(1)
    both = fetch(ctx, 1, plan, reads=False)
    for name in ("spectra_var", "sky_var", "channels_var", "channels", "spectra"):
        assert getattr(both, name).tobytes() == getattr(want, name).tobytes(), name
    ctx.set_channels(1, None)                                        # and without them again
    ctx.run(1)
    back = fetch(ctx, 1, plan, reads=False)
    assert back.channels_var is None and back.spectra_var.tobytes() == want.spectra_var.tobytes()
    # another read noise is another variance, by rn^2 q^2 per pixel
    ctx.set_variance(1, extraction.Variances(0.0))
    ctx.run(1)
    poisson = fetch(ctx, 1, plan, reads=False)
    rows = plan.row_windows[:, 1] - plan.row_windows[:, 0]
    # (column 0 is a border column: q = 1 and no sky template, so it holds rn^2 per row and nothing else of rn)
    assert np.allclose((want.spectra_var - poisson.spectra_var)[:, 0], RN * RN * rows, rtol=1e-9, atol=0.0)
    assert (poisson.spectra_var < want.spectra_var).all()


def test_refusals_leave_the_slot_extracting_without_variances():
    v = visit("small256")
    ctx = engine_of(v).ctx
    nothing, _ = descriptor(v, 1, None)
    ctx.upload(0, nothing)
    with pytest.raises(_lib.WayneError) as e:                        # no extraction on the slot
        ctx.set_variance(0, True)
    assert e.value.status == _lib.E_STATE
    with pytest.raises(_lib.WayneError) as e:                        # a slot that was never uploaded
        ctx.set_variance(202, True)
    assert e.value.status == _lib.E_STATE
    plain, gen = descriptor(v, 1, True)
    ctx.upload(1, plain)
    ctx.run(1)
    never, never_sky = ctx.download_spectra(1)

    def raw(slot, rn):
        d = _lib.VarianceDesc(rn)
        return ctx._L.wayne_exposure_set_variance(ctx._h, slot, C.byref(d))

    for rn in (-1.0, -1e-300, float("nan"), float("inf"), -float("inf")):
        ctx.upload(0, plain)
        ctx.set_variance(0, True)
        assert raw(0, rn) == _lib.E_INVALID, rn
    ctx.run(0)                                                       # ... and the slot extracts, without variances
    got, got_sky = ctx.download_spectra(0)
    assert got.tobytes() == never.tobytes() and got_sky.tobytes() == never_sky.tobytes()
    ps = [_lib._dp() for _ in range(3)]
    assert ctx._L.wayne_exposure_variances(ctx._h, 0, *[C.byref(p) for p in ps]) == _lib.E_STATE
    # the gain step off: refused like the rejection, the slot stays usable
    no_gain, gen_ng = descriptor(v, 1, extraction.ExtractionOptions(steps=extraction.ALL & ~extraction.GAIN))
    ctx.upload(0, no_gain)
    assert raw(0, 20.0) == _lib.E_INVALID
    with pytest.raises(_lib.WayneError) as e:
        ctx.set_variance(0, True)
    assert e.value.status == _lib.E_INVALID and not ctx.has_variance(0)
    ctx.run(0)
    assert np.isfinite(ctx.download_spectra(0)[0]).all()
    # the variances exist once the spectra have been fetched
    ctx.upload(0, plain)
    assert raw(0, 0.0) == 0
    ctx.set_variance(0, True)
    ctx.run(0)
    with pytest.raises(_lib.WayneError) as e:
        ctx.variances(0)
    assert e.value.status == _lib.E_STATE
    ctx.download_spectra(0)
    sv, kv, cv = ctx.variances(0)
    assert sv.shape == (v.NSAMP, 266) and kv.shape == (v.NSAMP,) and cv is None


def ensemble(v, n, channels, rn=RN, **over):
    """n exposures of `v` that differ in the generator's exposure index -- its random draws -- alone, each extracted with
    `channels` twice: with read noise rn and with none (the second run of a slot synthesises the same reads) ->
    (channels, channels_var, channels_var at read_noise 0) [n, R + 1, C]."""
    ctx = engine_of(v).ctx
    px = 2.0 ** -7
    S = planes(v).S
    sol = (np.full(S, 0.5), np.full(S, px))
    kw = v.frame_kwargs(0, cosmic_rate=None, ssv_generator=None, **over)
    out = []
    for i in range(n):
        gen = helpers.product_generator(v, i)
        desc = gen.build_descriptor(engine_of(v), extraction=extraction.ExtractionOptions(), **kw)
        plan = gen.extraction_plan.with_channels(channels, sol).with_variance(extraction.Variances(rn))
        ctx.upload(0, desc)
        ctx.set_extraction(0, plan)
        ctx.run(0)
        a = fetch(ctx, 0, plan, reads=False)
        ctx.set_variance(0, extraction.Variances(0.0))
        ctx.run(0)
        b = fetch(ctx, 0, plan, reads=False)
        assert a.channels.tobytes() == b.channels.tobytes()
        out.append((a.channels, a.channels_var, b.channels_var))
    return tuple(np.array([o[k] for o in out]) for k in range(3))


def test_the_law_describes_the_simulators_noise():
    """Does the law describe the simulator?  64 exposures of small256 that differ in their random draws alone (no cosmic
    rays, no scan-speed variation, no flat), 10 channels with edges on integer columns inside the trace (w is 0 or 1, the
    channels share no pixel).  Per channel: the ensemble variance of channels[:R].sum(0) over the ensemble mean of its
    predicted variance -- the intervals' Poisson parts plus the read noise of the last-read product, since consecutive
    intervals share a read (variance_law.ensemble_ratio) --, pooled over the channels: 630 times the pooled ratio is
    chi-square with 630 degrees of freedom, standard deviation sqrt(2 / 630) = 0.056 (derived, not measured); the test
    allows 4 of them.  Negative control: at read_noise = 0 the ratio must fall outside (a 60-row window's read noise is
    several times the photon noise here).  The same ensemble on CPU-oracle reads gave 0.918 and, without the read noise,
    2.668 (tests/test_variance.py); the figures measured on the device are in the README."""
    v = visit("small256")
    n = 64
    px = 2.0 ** -7
    edges = 0.5 + px * np.arange(59.0, 190.0, 13.0)                  # columns 59, 72, ... 189: inside the first order
    channels, cv, cv0 = ensemble(v, n, extraction.Channels(edges, flat=False), add_flat=False)
    R = v.NSAMP - 1
    sd = np.sqrt(2.0 / (10 * (n - 1)))
    ratio, per_channel = variance_law.ensemble_ratio(channels, cv, cv0)
    ratio0, _ = variance_law.ensemble_ratio(channels, cv0, cv0)
    naive = float((channels[:, :R].sum(axis=1).var(axis=0, ddof=1) / cv[:, :R].sum(axis=1).mean(axis=0)).mean())
    last = float((channels[:, R].var(axis=0, ddof=1) / cv[:, R].mean(axis=0)).mean())
    print("device, %d exposures: ensemble / predicted variance %.3f (per channel %s); with read_noise = 0: %.3f; "
          "allowed |ratio - 1| <= %.3f.  Not asserted: the intervals' variances added as they are %.3f, the last-read "
          "product alone %.3f" % (n, ratio, np.round(per_channel, 2), ratio0, 4 * sd, naive, last))
    # reported, not asserted: the flat in the reads and divided out again
    f_channels, f_cv, f_cv0 = ensemble(v, n, extraction.Channels(edges, flat=True), add_flat=True)
    print("device, flat on (add_flat=True, Channels(flat=True)): %.3f, with read_noise = 0: %.3f" % (
        variance_law.ensemble_ratio(f_channels, f_cv, f_cv0)[0], variance_law.ensemble_ratio(f_channels, f_cv0, f_cv0)[0]))
    assert (channels[:, :R].sum(axis=1).mean(axis=0) > 1e5).all()    # the channels do lie on the trace
    assert abs(ratio - 1.0) <= 4 * sd
    assert abs(ratio0 - 1.0) > 4 * sd


def test_frames_visits_and_observations_carry_the_variances():
    v = visit("tiny")
    ch = extraction.Channels.linear(1.0, 1.8, 12)
    exp = helpers.product_generator(v, 0).scanning_frame(extraction=True, channels=ch, variance=True, **v.frame_kwargs(0))
    assert exp.spectra_var.shape == (4, 74) and exp.sky_var.shape == (4,) and exp.channels_var.shape == (4, 12)
    assert exp.extraction.variance.read_noise == 20.0
    plain = helpers.product_generator(v, 0).scanning_frame(extraction=True, channels=ch, **v.frame_kwargs(0))
    assert not hasattr(plain, "spectra_var") and plain.spectra.tobytes() == exp.spectra.tobytes()
    assert plain.channels.tobytes() == exp.channels.tobytes()
    run = Run(np.stack([r[0] for r in exp.reads]), exp.spectra, exp.sky, exp.channels, None, exp.spectra_var, exp.sky_var,
              exp.channels_var, exp.extraction)
    assert_is_the_law(run, v, "scanning_frame(variance=True)")
    alone = helpers.product_generator(v, 0).scanning_frame(extraction=True, variance=extraction.Variances(20.0), **v.frame_kwargs(0))
    assert alone.channels_var is None and alone.spectra_var.tobytes() == exp.spectra_var.tobytes()

    runner = VisitRunner(v)
    spectra, sky = runner.run_spectra(range(3), extraction=extraction.ExtractionOptions(channels=ch, variance=True))
    assert runner.spectra_var.shape == (3, 4, 74) and runner.sky_var.shape == (3, 4) and runner.channels_var.shape == (3, 4, 12)
    assert runner.spectra_var[0].tobytes() == exp.spectra_var.tobytes() and runner.channels_var[0].tobytes() == exp.channels_var.tobytes()
    runner.run_spectra(range(2), extraction=extraction.ExtractionOptions(variance=True))
    assert runner.channels_var is None and runner.spectra_var[0].tobytes() == exp.spectra_var.tobytes()
    runner.run_spectra(range(2))
    assert runner.spectra_var is None and runner.sky_var is None and runner.channels_var is None
    runner.run(range(2), extraction=extraction.ExtractionOptions(channels=ch, variance=True))
    assert sorted(runner.spectra_var) == [0, 1] and runner.channels_var[0].tobytes() == exp.channels_var.tobytes()
    assert runner.sky_var[0].tobytes() == exp.sky_var.tobytes()
    runner.run(range(1), extraction=True)
    assert runner.spectra_var is None

    s = visit("stare256")
    kw = s.frame_kwargs(0)
    for drop in ("scan_speed", "sample_rate", "ssv_generator"):
        kw.pop(drop, None)
    stare = helpers.product_generator(s, 0).staring_frame(extraction=True, variance=True, **kw)
    assert stare.spectra_var.shape == (4, 266) and stare.spectra_var.max() > 1e4 and stare.channels_var is None


def test_cli_writes_the_variances_and_they_are_the_frames(tmp_path):
    work = str(tmp_path / "visit")
    shutil.copytree(MINI, work)
    yml = os.path.join(work, "params.yml")
    out, plain, both = str(tmp_path / "var.npz"), str(tmp_path / "plain.npz"), str(tmp_path / "both.npz")
    base = ["spectra", "sky", "exposure_index", "row_lo", "row_hi", "bg_cols", "x_ref", "y_ref", "read_times", "exp_start"]
    obs = run_visit.run(["-p", yml, "--max-exposures", "3", "--spectra-only", out, "--variances"])
    z = np.load(out)
    assert sorted(z.files) == sorted(base + ["spectra_var", "sky_var", "variance_read_noise"])
    n, NP, S = z["spectra"].shape
    assert z["spectra_var"].shape == (3, NP, S) and z["sky_var"].shape == (3, NP) and float(z["variance_read_noise"]) == 20.0
    np.testing.assert_array_equal(z["spectra_var"], obs.spectra_result["spectra_var"])
    assert (z["spectra_var"][:, :NP - 1] > 0.0).all()
    obs2 = run_visit.run(["-p", yml, "--max-exposures", "3", "--spectra-only", plain])
    zp = np.load(plain)
    assert sorted(zp.files) == sorted(base) and "spectra_var" not in obs2.spectra_result
    assert zp["spectra"].tobytes() == z["spectra"].tobytes() and zp["sky"].tobytes() == z["sky"].tobytes()
    # Observation.frame_options["variance"] through the frame API: the same exposure, the same bytes
    obs2.frame_options["variance"] = True
    obs2.spectra_out, obs2.spectra_only = None, False
    frame = obs2._generate_exposure(obs2.exp_start_times[1], 2, write_fits=False)
    assert frame.spectra_var.tobytes() == z["spectra_var"][1].tobytes() and frame.sky_var.tobytes() == z["sky_var"][1].tobytes()
    run_visit.run(["-p", yml, "--max-exposures", "2", "--spectra-only", both, "--variances", "12.5", "--channels", "1.1:1.7:20",
                   "--reject-cosmics"])
    zb = np.load(both)
    assert sorted(zb.files) == sorted(base + ["spectra_var", "sky_var", "channels_var", "variance_read_noise", "channels",
                                              "channel_edges_um", "channel_flat", "wl_a", "wl_b", "n_rejected", "crrej_k",
                                              "crrej_read_noise"])
    assert zb["channels_var"].shape == (2, NP, 20) and float(zb["variance_read_noise"]) == 12.5
    assert (zb["spectra_var"][:, :NP - 1] < z["spectra_var"][:2, :NP - 1]).any()
