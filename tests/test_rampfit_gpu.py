"""GPU: the ramp fit (wayne_exposure_set_rampfit, k_ramp_fit, --rate-images).

The law is tests/rampfit_law.py, applied to the slot's own downloaded reads.  Bounds (derived there, not tuned):
  * word equal, except for pixels whose deciding z_j* lies within 1e-9 relative of k_jump in the law -- printed, and no
    more than 1e-4 of the pixels (none is expected);
  * where the word agrees, |rate - law| <= 1e-9 M, M = (sum |w_j d_j| + |rate| sum |w_j| dt_j) / |den|; var to 4e-9 of itself;
  * bytes: equal planes in slots 0 and 5 (the other stream) and on a second run; reads and spectra bit-identical with the
    option on and off;
  * noise: 32 exposures of stare16_128 that differ in their draws alone -- the mean over the pixels at >= 5 e-/s of
    ensemble variance / mean predicted variance within 1 +- 4 sqrt(2 / (n_pix 31)); with read_noise near 0 outside.
CPU side (the law itself, the CPU-oracle ensembles, host validation): tests/test_rampfit.py."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import extraction_law
import helpers
import rampfit_law as law
from fits_words_law import clock_free
from wayne_amd import _lib, engine, fitsio, rampfit, run_visit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI = os.path.join(ROOT, "tests", "fixtures", "mini_visit")
_visits, _planes = {}, {}
# (configuration, E): R = 3; R = 2, so the jump test is never entered; R = 4; a scan over 15 intervals -- and the same scan
# a hundred times brighter, where the star crossing a pixel stands out of the read noise and thousands of pixels lose
# several intervals: the hard case for the jump loop (at the configuration's own 3e5 electrons a dozen pixels are
# flagged); the staring ramp, and the same with saturated pixels
CASES = [("tiny", None), ("tiny_g102", None), ("tiny128", None), ("ramp16_128", None), ("ramp16_128", 3e7),
         ("stare16_128", None), ("stare16_128", 1.2e8)]
IDS = ["tiny", "tiny_g102", "tiny128", "ramp16_128", "ramp16_128_bright", "stare16_128", "stare16_128_bright"]


def visit(name, E=None, n=1):
    key = (name, E, n)
    if key not in _visits:
        _visits[key] = helpers.make_visit(name, n_exposures=n, **({"E": E} if E else {}))
    return _visits[key]


def planes(v):
    if v.name not in _planes:
        _planes[v.name] = extraction_law.Planes(v)
    return _planes[v.name]


def engine_of(v):
    return engine.get_engine(0, v.grism, v.detector, v.calibration, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)


def descriptor(v, i=0, out_dtype=np.float32, **over):
    opts = {k: over.pop(k) for k in list(over) if k in ("ramp_fit", "extraction", "rng_mode")}
    gen = helpers.product_generator(v, i)
    return gen.build_descriptor(engine_of(v), out_dtype=out_dtype, **opts, **v.frame_kwargs(i, **over))


def fitted(v, fit, out_dtype=np.float32, slot=0, i=0, **over):
    """(reads, (rate, var, word)) of exposure i run in `slot` with the ramp fit `fit`."""
    ctx = engine_of(v).ctx
    ctx.upload(slot, descriptor(v, i, out_dtype, ramp_fit=fit, **over))
    assert ctx.has_rampfit(slot)
    ctx.run_checked(slot)
    return ctx.download(slot).copy(), ctx.rampfit(slot)


def assert_is_the_law(v, reads, got, fit, what):
    want = law.restate(reads, planes(v), fit.read_noise, fit.k, fit.saturation_dn, fit.steps)
    law.assert_parity(got[0], got[1], got[2], want, what)
    return want


# ---- a. parity with the law -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", [np.float32, np.float64, np.uint16], ids=["f32", "f64", "u16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_device_fits_the_law(case, out_dtype):
    name, E = case
    v = visit(name, E)
    fit = rampfit.RampFit()
    reads, got = fitted(v, fit, out_dtype)
    assert reads.dtype == out_dtype
    want = assert_is_the_law(v, reads, got, fit, "%s %s" % (IDS[CASES.index(case)], np.dtype(out_dtype).name))
    R = v.NSAMP - 1
    K = want.word[5:-5, 5:-5] >> 16
    assert want.rate.max() > 1.0                                            # (the comparison is not one of zeros)
    if name == "tiny_g102":
        assert R == 2 and not want.jump.any() and np.isinf(want.margin).all()      # the jump test is never entered
    if name == "ramp16_128" and E:
        lost = np.array([bin(int(j)).count("1") for j in want.jump.ravel()])
        assert (lost >= 3).sum() >= 100                                     # (the CPU oracle's exposure: 4012 pixels)
    elif E:
        assert (K < R).sum() >= 100 and (K > 0).all() if out_dtype != np.uint16 else (K < R).sum() >= 100
    elif name == "stare16_128":
        assert (K == R).all()


@pytest.mark.parametrize("variant", ["k0", "no_linearise", "no_dark", "own"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_options_are_the_laws(case, variant):
    name, E = case
    v = visit(name, E)
    fit = {"k0": rampfit.RampFit(k=0.0), "no_linearise": rampfit.RampFit(linearise=False),
           "no_dark": rampfit.RampFit(dark=False), "own": rampfit.RampFit(read_noise=12.5, k=3.5, saturation_dn=20000.0)}[variant]
    reads, got = fitted(v, fit, slot=3)
    want = assert_is_the_law(v, reads, got, fit, "%s %s" % (IDS[CASES.index(case)], variant))
    if variant == "k0":
        assert not (got[2] & 0xFFFF).any() and np.isinf(want.margin).all()
    if variant == "own" and E and name == "stare16_128":
        assert ((want.word[5:-5, 5:-5] >> 16) == 0).any() or ((want.word[5:-5, 5:-5] >> 16) < 15).sum() > 200


def test_samples_behind_a_saturated_one_are_not_used_again():
    # The simulator's ramps rise, so a read below saturation_dn behind one above it needs a threshold inside the noise: the
    # median of the sky pixels' eighth read.  The sky adds 17 DN an interval and a difference of two reads has 8.5 DN of
    # noise, so a few per cent of the pixels that cross there dip below the threshold once more.
    v = visit("stare16_128")
    ctx = engine_of(v).ctx
    ctx.upload(2, descriptor(v))
    ctx.run_checked(2)
    reads = ctx.download(2).copy()
    sat = float(np.median(reads[8, 5:-5, 5:-5]))
    fit = rampfit.RampFit(saturation_dn=sat)
    ctx.set_rampfit(2, fit)
    ctx.run_checked(2)
    np.testing.assert_array_equal(ctx.download(2).view(np.uint32), reads.view(np.uint32))
    want = assert_is_the_law(v, reads, ctx.rampfit(2), fit, "stare16_128 saturating at its eighth read's median")
    good = reads[:, 5:-5, 5:-5].astype(np.float64) < sat
    K = want.word[5:-5, 5:-5] >> 16
    again = (good.sum(axis=0) - 1 > K) & good[0]          # a good sample behind the first bad one
    print("%d pixels hold a sample below %.1f DN behind one above it" % (int(again.sum()), sat))
    assert again.sum() >= 30 and len(np.unique(K)) >= 8


def test_replay_mode_is_admitted():
    v = visit("tiny")
    fit = rampfit.RampFit()
    reads, got = fitted(v, fit, rng_mode=_lib.RNG_REPLAY)
    assert_is_the_law(v, reads, got, fit, "tiny replay")


# ---- b. bytes -------------------------------------------------------------------------------------------------------
def test_the_same_bytes_everywhere_and_nothing_else_changes():
    v = visit("stare16_128")
    ctx = engine_of(v).ctx
    with_fit = descriptor(v, ramp_fit=True, extraction=True)
    plain = descriptor(v, extraction=True)

    def run(slot, d):
        ctx.upload(slot, d)
        ctx.run_checked(slot)
        return ctx.download(slot).copy(), [a.copy() for a in ctx.download_spectra(slot)]

    def same(a, b):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))

    reads0, spectra0 = run(0, with_fit)
    p0 = ctx.rampfit(0)
    assert p0[0].max() > 100.0 and (p0[2] >> 16).max() == 15
    ctx.run_checked(0)                                   # a second run of the same upload
    same(ctx.rampfit(0), p0)
    reads5, _ = run(5, with_fit)                         # another slot, the other stream
    same(ctx.rampfit(5), p0)
    # an upload without the option: no planes any more, and reads and spectra as with it
    reads_p, spectra_p = run(0, plain)
    assert not ctx.has_rampfit(0)
    with pytest.raises(_lib.WayneError) as e:
        ctx.rampfit(0)
    assert e.value.status == _lib.E_STATE
    same([reads_p, reads5], [reads0, reads0])
    same(spectra_p, spectra0)
    run(0, with_fit)
    same(ctx.rampfit(0), p0)
    # the fit's own profile slot counts its launches, and the default path launches none
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        run(0, plain)
        assert ctx.rampfit_profile()["launches"] == 0
        run(0, with_fit)
        prof = ctx.rampfit_profile()
        assert prof["launches"] == 1 and prof["ms"] > 0.0
    finally:
        ctx.profile_enable(False)


# ---- c. errors ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_slot_running_without_the_fit():
    v = visit("tiny")
    eng = engine_of(v)
    ctx = eng.ctx
    L, hnd = ctx._L, ctx._h
    S = eng.S
    rate, var, word = np.empty((S, S)), np.empty((S, S)), np.empty((S, S), dtype=np.uint32)
    out = (_lib.ptr(rate, C.c_double), _lib.ptr(var, C.c_double), _lib.ptr(word, C.c_uint32))
    ctx.upload(7, descriptor(v))
    ctx.run_checked(7)
    want = ctx.download(7).copy()
    assert L.wayne_exposure_download_rampfit(hnd, 7, *out) == _lib.E_STATE            # without the option
    nan, inf = float("nan"), float("inf")
    for bad in ((3, 20.0, 5.0, 65000.0), (0, 20.0, 5.0, 65000.0), (7 | 8, 20.0, 5.0, 65000.0), (7 | 16, 20.0, 5.0, 65000.0),
                (7, 0.0, 5.0, 65000.0), (7, -1.0, 5.0, 65000.0), (7, nan, 5.0, 65000.0), (7, inf, 5.0, 65000.0),
                (7, 20.0, -1.0, 65000.0), (7, 20.0, nan, 65000.0), (7, 20.0, inf, 65000.0),
                (7, 20.0, 5.0, 0.0), (7, 20.0, 5.0, -1.0), (7, 20.0, 5.0, nan), (7, 20.0, 5.0, inf)):
        ctx.set_rampfit(7, True)
        assert ctx.has_rampfit(7)
        d = _lib.RampFitDesc(*bad)
        assert L.wayne_exposure_set_rampfit(hnd, 7, C.byref(d)) == _lib.E_INVALID, bad
        assert L.wayne_exposure_download_rampfit(hnd, 7, *out) == _lib.E_STATE, bad   # the refusal cleared the option
    for slot in (-1, 10000):
        assert L.wayne_exposure_set_rampfit(hnd, slot, C.byref(_lib.RampFitDesc(7, 20.0, 5.0, 65000.0))) == _lib.E_INVALID
    # a slot that is not uploaded
    ok = _lib.RampFitDesc(7, 20.0, 5.0, 65000.0)
    assert L.wayne_exposure_set_rampfit(hnd, 200, C.byref(ok)) == _lib.E_STATE
    assert L.wayne_exposure_download_rampfit(hnd, 200, *out) == _lib.E_STATE
    # the slot runs on, without the fit
    ctx._slot_rampfit.pop(7, None)
    ctx.run_checked(7)
    np.testing.assert_array_equal(ctx.download(7), want)
    # the option still works on the slot afterwards: not before a run, then the law, then cleared by NULL and by an upload
    ctx.set_rampfit(7, True)
    assert L.wayne_exposure_download_rampfit(hnd, 7, *out) == _lib.E_STATE            # set, but not run yet
    ctx.run_checked(7)
    got = ctx.rampfit(7)
    np.testing.assert_array_equal(ctx.download(7), want)
    assert_is_the_law(v, want, got, rampfit.RampFit(), "tiny after the refusals")
    ctx.set_rampfit(7, None)
    assert not ctx.has_rampfit(7) and L.wayne_exposure_download_rampfit(hnd, 7, *out) == _lib.E_STATE
    ctx.set_rampfit(7, True)
    ctx.upload(7, descriptor(v))
    assert not ctx.has_rampfit(7) and L.wayne_exposure_download_rampfit(hnd, 7, *out) == _lib.E_STATE


# ---- d. the public path ---------------------------------------------------------------------------------------------
def staring_kwargs(v, i=0, **over):
    kw = v.frame_kwargs(i, **over)
    return {k: kw[k] for k in kw if k not in ("scan_speed", "sample_rate", "ssv_generator")}


def test_staring_frame_carries_the_rate_image():
    v = visit("stare16_128")
    frame = helpers.product_generator(v, 0).staring_frame(ramp_fit=True, **staring_kwargs(v))
    ctx = engine_of(v).ctx
    S = v.detector.full_size(v.SUBARRAY)
    assert frame.rate.shape == frame.rate_var.shape == frame.rate_word.shape == (S, S)
    assert frame.rate.dtype == frame.rate_var.dtype == np.float64 and frame.rate_word.dtype == np.uint32
    for a, b in zip((frame.rate, frame.rate_var, frame.rate_word), ctx.rampfit(0)):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    reads = np.stack([np.asarray(r) for r, _ in frame.reads])
    assert_is_the_law(v, reads, (frame.rate, frame.rate_var, frame.rate_word), rampfit.RampFit(), "staring_frame")
    dq, nsamp, time = law.derived(frame.rate_word, planes(v).dt)
    assert (frame.rate_dq == dq).all() and (frame.rate_nsamp == nsamp).all() and np.allclose(frame.rate_time, time, rtol=1e-12)
    assert (frame.rate_nsamp[5:-5, 5:-5] >= 13).all() and not frame.rate_nsamp[:5].any()
    plain = helpers.product_generator(v, 0).staring_frame(**staring_kwargs(v))
    assert plain.rate is None and plain.rate_dq is None
    for (a, _), (b, _) in zip(frame.reads, plain.reads):
        np.testing.assert_array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def test_the_visit_runner_delivers_the_planes(tmp_path):
    from wayne_amd import visit as wv
    v = visit("tiny128", n=3)
    seen = {}
    runner = wv.VisitRunner(v, 0, out_dir=str(tmp_path / "with"))
    kept = runner.run(range(3), keep=True, ramp_fit=rampfit.RampFit(k=4.0), on_ramp_fit=lambda i, *p: seen.__setitem__(i, p))
    assert sorted(seen) == sorted(runner.ramp_fit) == [0, 1, 2]
    plain_runner = wv.VisitRunner(v, 0, out_dir=str(tmp_path / "plain"))
    plain = plain_runner.run(range(3), keep=True)
    assert plain_runner.ramp_fit is None
    for i in range(3):
        for a, b in zip(seen[i], runner.ramp_fit[i]):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(kept[i].view(np.uint32), plain[i].view(np.uint32))
        assert_is_the_law(v, kept[i], seen[i], rampfit.RampFit(k=4.0), "VisitRunner exposure %d" % i)
    names = sorted(os.listdir(str(tmp_path / "with")))
    assert [m for m in names if m.endswith("_rate.fits")] == ["%04d_rate.fits" % (i + 1) for i in range(3)]
    assert not [m for m in os.listdir(str(tmp_path / "plain")) if m.endswith("_rate.fits")]
    for m in (m for m in names if m.endswith("_raw.fits")):
        a = clock_free(open(str(tmp_path / "with" / m), "rb").read())
        b = clock_free(open(str(tmp_path / "plain" / m), "rb").read())
        assert a == b, m
    with pytest.raises(TypeError):
        wv.VisitRunner(v, 0).run(range(1), ramp_fit="yes")


def test_the_cli_writes_rate_files_beside_the_raw_files(tmp_path):
    n = 4
    outs = {}
    for flag in ((), ("--rate-images",), ("--rate-images", "0")):
        work = str(tmp_path / ("visit%d" % len(flag)))
        shutil.copytree(MINI, work)
        outs[flag] = run_visit.run(["-p", os.path.join(work, "params.yml"), "--max-exposures", str(n)] + list(flag))
    plain = outs[()]
    assert not [m for m in os.listdir(plain.outdir) if m.endswith("_rate.fits")]
    for flag, k in ((("--rate-images",), 5.0), (("--rate-images", "0"), 0.0)):
        obs = outs[flag]
        names = sorted(m for m in os.listdir(obs.outdir) if m.endswith("_rate.fits"))
        assert names == ["%04d_rate.fits" % (i + 1) for i in range(n)]
        R = obs.NSAMP - 1
        for i, m in enumerate(names):
            hdus = fitsio.read(os.path.join(obs.outdir, m))
            raw = fitsio.read(os.path.join(obs.outdir, "%04d_raw.fits" % (i + 1)))
            p = hdus[0].header
            assert p["RFRN"] == 20.0 and p["RFK"] == k and p["RFSAT"] == 65000.0 and hdus[0].data is None
            for key in raw[0].header.keys():
                if key not in ("DATE", "SIM-TIME", "COMMENT", "HISTORY", ""):
                    assert p[key] == raw[0].header[key], key
            assert [h.name for h in hdus[1:]] == ["SCI", "ERR", "DQ", "SAMP", "TIME"]
            assert [h.header["BITPIX"] for h in hdus[1:]] == [-32, -32, 16, 16, -32]
            assert all(h.header["EXTVER"] == 1 for h in hdus[1:])
            sci, err, dq, samp, time = (np.asarray(h.data) for h in hdus[1:])
            assert np.isfinite(sci).all() and sci.max() > 1.0 and (err[5:-5, 5:-5] > 0).all() and not sci[:5].any()
            assert samp.max() == R and (samp[5:-5, 5:-5] <= R).all() and time.max() > 0
            if k == 0.0:
                assert not (dq & 8192).any()
            # the _raw files keep their bytes
            a = clock_free(open(os.path.join(obs.outdir, "%04d_raw.fits" % (i + 1)), "rb").read())
            b = clock_free(open(os.path.join(plain.outdir, "%04d_raw.fits" % (i + 1)), "rb").read())
            assert a == b, m
    engine.close_all()


# ---- e. does the variance describe the device's noise? ---------------------------------------------------------------
def test_the_variance_describes_the_devices_noise():
    """32 exposures of stare16_128 that differ in their draws alone, no cosmic rays, every other noise source on (the
    pointing jitter too: the CPU-oracle ensemble of tests/test_rampfit.py passes with it).  A pixel's (n - 1) s^2 / sigma^2
    is chi-square with n - 1 degrees of freedom, so the mean over n_pix pixels of ensemble variance / mean predicted
    variance has standard deviation sqrt(2 / (n_pix (n - 1))): 4 of them are allowed -- derived, not measured.  The ratio
    is taken pixel by pixel: that is what the bound holds for.  Control: the same reads fitted with read_noise = 0.001."""
    n = 32
    v = visit("stare16_128", n=n)
    ctx = engine_of(v).ctx
    pl = planes(v)
    gen_kw = dict(cosmic_rate=None, x_ref=v.x_refs[0], y_ref=v.y_refs[0], sky_background=v.sky[0], scale_factor=1.0,
                  planet_signal=v.planet_signal(0))
    rates, variances, control = [], [], []
    for i in range(n):
        reads, got = fitted(v, rampfit.RampFit(), slot=i % 2, i=i, **gen_kw)
        rates.append(got[0]); variances.append(got[1])
        control.append(law.restate(reads, pl, rn=1e-3).var)
    rates = np.array(rates)
    ratio, n_pix = law.ensemble_ratio(rates, np.array(variances))
    ratio0, _ = law.ensemble_ratio(rates, np.array(control))
    bound = 4 * np.sqrt(2.0 / (n_pix * (n - 1)))
    print("device, %d exposures of stare16_128, %d pixels at >= 5 e-/s: ensemble / predicted variance %.4f (allowed 1 +- %.4f); "
          "with read_noise = 0.001: %.3f" % (n, n_pix, ratio, bound, ratio0))
    assert n_pix >= 100
    assert abs(ratio - 1.0) <= bound
    assert abs(ratio0 - 1.0) > bound
