"""GPU: the calibrated reads (wayne_exposure_set_ima, k_ima, --ima).

The law is tests/ima_law.py, applied to the slot's own downloaded reads (and, with a ramp fit on the slot, to the word the
device's ramp fit delivered for the same run).  Tolerance: none -- the device's payload equals the law's byte for byte,
padding included (derived in ima_law's docstring; NaN samples, of which these cases have none, compared as NaN).
  * bytes: equal payloads in slots 0 and 5 (the other stream) and on a second run; reads, spectra and rate planes
    bit-identical with the option on and off;
  * what an observer does with the file: on small256 the column sums of SCI_{j+1} - SCI_j of a counts-unit payload over
    the plan's window equal the device's own spectra_j within the float32 storage alone,
    2^-24 sum_y (|e_{j+1}| + |e_j|) per column.
CPU side (the layout, the law against the laws it borrows from, host validation, the file): tests/test_ima.py."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import extraction_law
import helpers
import ima_law as law
from fits_words_law import clock_free
from wayne_amd import _lib, engine, extraction, fitsio, ima, rampfit, run_visit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI = os.path.join(ROOT, "tests", "fixtures", "mini_visit")
_visits, _planes = {}, {}
# (configuration, E): R = 3 on 74^2; R = 2; R = 4 on 138^2; all 15 intervals, a scan and a staring ramp, and that ramp with
# hundreds of pixels cut short (K < R); the full array, the only frame whose DQ section ends on a whole 16-byte vector
CASES = [("tiny", None), ("tiny_g102", None), ("tiny128", None), ("ramp16_128", None), ("stare16_128", None),
         ("stare16_128", 1.2e8), ("full3", None)]
IDS = ["tiny", "tiny_g102", "tiny128", "ramp16_128", "stare16_128", "stare16_128_bright", "full3"]


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
    opts = {k: over.pop(k) for k in list(over) if k in ("ima", "ramp_fit", "extraction", "rng_mode")}
    gen = helpers.product_generator(v, i)
    return gen.build_descriptor(engine_of(v), out_dtype=out_dtype, **opts, **v.frame_kwargs(i, **over))


def formed(v, opt, out_dtype=np.float32, slot=0, i=0, **over):
    """(reads, payload bytes, the ramp fit's word or None) of exposure i run in `slot` with the calibrated reads `opt`."""
    ctx = engine_of(v).ctx
    ctx.upload(slot, descriptor(v, i, out_dtype, ima=opt, **over))
    assert ctx.has_ima(slot)
    ctx.run_checked(slot)
    word = ctx.rampfit(slot)[2] if ctx.has_rampfit(slot) else None
    return ctx.download(slot).copy(), ctx.ima(slot), word


def assert_is_the_law(v, reads, got, opt, what, word=None):
    want = law.restate(reads, planes(v), opt.units, opt.read_noise, opt.saturation_dn, opt.steps, jump=word)
    assert got.layout == ima.layout(reads.shape[-1], reads.shape[0] - 1)
    law.assert_parity(got.bytes, want, what)
    return want


# ---- a. parity with the law -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("units", ["rate", "counts"])
@pytest.mark.parametrize("out_dtype", [np.float32, np.float64, np.uint16], ids=["f32", "f64", "u16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_device_forms_the_law(case, out_dtype, units):
    name, E = case
    v = visit(name, E)
    opt = ima.Ima(units)
    reads, got, _ = formed(v, opt, out_dtype)
    assert reads.dtype == out_dtype
    want = assert_is_the_law(v, reads, got, opt, "%s %s %s" % (IDS[CASES.index(case)], np.dtype(out_dtype).name, units))
    R, S = v.NSAMP - 1, reads.shape[-1]
    assert want.sci[R].max() > 1.0 and (want.err[1:, 5:-5, 5:-5] > 0).all()          # (the comparison is not one of zeros)
    assert (S * S % 8 == 0) == (name == "full3")
    if E:
        cut = want.K[5:-5, 5:-5] < R
        assert cut.sum() >= 100 and ((want.dq[R] & 256) != 0).sum() == cut.sum() and not (want.dq[1] & 256).all()
    elif name == "stare16_128":
        assert not want.dq.any()
    # the views of the payload are the law's planes
    for k in (0, R):
        assert (got.sci(k).view(np.uint32) == want.sci[k].astype(">f4").view(np.uint32)).all() and (got.dq(k) == want.dq[k]).all()
        assert np.shares_memory(got.err(k), got.bytes)


@pytest.mark.parametrize("variant", ["no_linearise", "no_dark", "own", "sat20000"])
@pytest.mark.parametrize("case", [("tiny128", None), ("stare16_128", None)], ids=["tiny128", "stare16_128"])
def test_the_options_are_the_laws(case, variant):
    name, E = case
    v = visit(name, E)
    opt = {"no_linearise": ima.Ima(linearise=False), "no_dark": ima.Ima("counts", dark=False),
           "own": ima.Ima("counts", read_noise=12.5, saturation_dn=31000.0),
           "sat20000": ima.Ima("rate", saturation_dn=20000.0)}[variant]
    reads, got, _ = formed(v, opt, slot=3)
    want = assert_is_the_law(v, reads, got, opt, "%s %s" % (name, variant))
    full = law.restate(reads, planes(v), opt.units)
    if variant in ("no_linearise", "no_dark"):
        assert (want.sci != full.sci).any()                                # the step does something on these reads
    if variant == "own":
        assert (want.err != law.restate(reads, planes(v), "counts").err).any()
    if variant == "sat20000" and name == "stare16_128":
        K = want.K[5:-5, 5:-5]
        print("stare16_128 at 20000 DN: %d pixels cut short, %d at K = 0" % (int((K < 15).sum()), int((K == 0).sum())))
        assert (K < 15).sum() >= 50 and ((want.dq & 256) != 0).any()


def test_a_read_below_saturation_behind_one_above_it_stays_flagged():
    # The simulator's ramps rise, so a read below saturation_dn behind one above it needs a threshold inside the noise: the
    # median of the sky pixels' eighth read (tests/test_rampfit_gpu.py has the arithmetic).
    v = visit("stare16_128")
    ctx = engine_of(v).ctx
    ctx.upload(2, descriptor(v))
    ctx.run_checked(2)
    reads = ctx.download(2).copy()
    sat = float(np.median(reads[8, 5:-5, 5:-5]))
    opt = ima.Ima("counts", saturation_dn=sat)
    ctx.set_ima(2, opt)
    ctx.run_checked(2)
    np.testing.assert_array_equal(ctx.download(2).view(np.uint32), reads.view(np.uint32))
    want = assert_is_the_law(v, reads, ctx.ima(2), opt, "stare16_128 saturating at its eighth read's median")
    good = reads[:, 5:-5, 5:-5].astype(np.float64) < sat
    flagged = (want.dq[:, 5:-5, 5:-5] & 256) != 0
    again = good[1:] & flagged[1:]                         # a read below the threshold that carries 256 all the same
    print("%d reads below %.1f DN behind one above it" % (int(again.sum()), sat))
    assert again.sum() >= 30 and len(np.unique(want.K[5:-5, 5:-5])) >= 8


def test_reads_behind_a_jump_of_the_slots_ramp_fit_carry_8192():
    v = visit("stare16_128")
    opt = ima.Ima()
    # cosmic rays on (the visit's 11 per second), a ramp fit with its jump test on: 8192 behind every cut interval
    reads, got, word = formed(v, opt, slot=1, ramp_fit=rampfit.RampFit())
    assert word is not None and (word & 0xFFFF).any()
    want = assert_is_the_law(v, reads, got, opt, "stare16_128 with a ramp fit", word)
    n_jump = int(((want.dq[15] & 8192) != 0).sum())
    assert n_jump == int(((word & 0xFFFF) != 0).sum()) >= 5 and not (want.dq[0] & 8192).any()
    # the ramp fit's own saturation_dn is not this option's: both flags come from their own rule
    reads2, got2, word2 = formed(v, ima.Ima(saturation_dn=20000.0), slot=1, ramp_fit=rampfit.RampFit(saturation_dn=30000.0))
    assert_is_the_law(v, reads2, got2, ima.Ima(saturation_dn=20000.0), "two thresholds", word2)
    # its k = 0: a word without jump bits, no 8192 anywhere
    reads0, got0, word0 = formed(v, opt, slot=1, ramp_fit=rampfit.RampFit(k=0.0))
    assert not (word0 & 0xFFFF).any()
    want0 = assert_is_the_law(v, reads0, got0, opt, "stare16_128 with a ramp fit, k = 0", word0)
    assert not (want0.dq & 8192).any()
    # no ramp fit on the slot: none either, and the samples are the same
    reads_n, got_n, word_n = formed(v, opt, slot=1)
    assert word_n is None
    want_n = assert_is_the_law(v, reads_n, got_n, opt, "stare16_128 without a ramp fit")
    assert not (want_n.dq & 8192).any()
    np.testing.assert_array_equal(reads_n.view(np.uint32), reads.view(np.uint32))
    assert (want_n.sci.view(np.uint32) == want.sci.view(np.uint32)).all()
    # the ramp fit cleared on a slot that keeps the option: no stale word is read
    ctx = engine_of(v).ctx
    ctx.upload(1, descriptor(v, ima=opt, ramp_fit=rampfit.RampFit()))
    ctx.set_rampfit(1, None)
    ctx.run_checked(1)
    assert_is_the_law(v, ctx.download(1).copy(), ctx.ima(1), opt, "ramp fit cleared")


def test_replay_mode_is_admitted():
    v = visit("tiny")
    opt = ima.Ima("counts")
    reads, got, _ = formed(v, opt, rng_mode=_lib.RNG_REPLAY)
    assert_is_the_law(v, reads, got, opt, "tiny replay")


# ---- b. bytes -------------------------------------------------------------------------------------------------------
def test_the_same_bytes_everywhere_and_nothing_else_changes():
    v = visit("stare16_128")
    ctx = engine_of(v).ctx
    with_ima = descriptor(v, ima="rate", ramp_fit=True, extraction=True)
    plain = descriptor(v, ramp_fit=True, extraction=True)

    def run(slot, d):
        ctx.upload(slot, d)
        ctx.run_checked(slot)
        return ctx.download(slot).copy(), [a.copy() for a in ctx.download_spectra(slot)], ctx.rampfit(slot)

    def same(a, b):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))

    reads0, spectra0, fit0 = run(0, with_ima)
    p0 = ctx.ima(0)
    assert p0.sci(15).max() > 100.0
    ctx.run_checked(0)                                   # a second run of the same upload
    same([ctx.ima(0).bytes], [p0.bytes])
    reads5, _, _ = run(5, with_ima)                      # another slot, the other stream
    same([ctx.ima(5).bytes], [p0.bytes])
    # an upload without the option: no payload any more, and reads, spectra and rate planes as with it
    reads_p, spectra_p, fit_p = run(0, plain)
    assert not ctx.has_ima(0)
    with pytest.raises(_lib.WayneError) as e:
        ctx.ima(0)
    assert e.value.status == _lib.E_STATE
    same([reads_p, reads5], [reads0, reads0])
    same(spectra_p, spectra0)
    same(fit_p, fit0)
    run(0, with_ima)
    same([ctx.ima(0).bytes], [p0.bytes])
    # the kernel's own profile slot counts its launches, and the default path launches none
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        run(0, plain)
        assert ctx.ima_profile()["launches"] == 0
        run(0, with_ima)
        prof = ctx.ima_profile()
        assert prof["launches"] == 1 and prof["ms"] > 0.0
    finally:
        ctx.profile_enable(False)


def test_the_padding_is_written_on_every_run():
    # the buffer is first filled by a run in the other unit, whose samples have no zero byte to lend; then the option is set
    # again on the same slot, in this unit: the payload is the law's, its padding zero
    v = visit("tiny128")
    ctx = engine_of(v).ctx
    ctx.upload(4, descriptor(v, ima="counts"))
    ctx.run_checked(4)
    first = ctx.ima(4)
    assert first.bytes.any()
    opt = ima.Ima("rate")
    ctx.set_ima(4, opt)
    ctx.run_checked(4)
    got = ctx.ima(4)
    want = assert_is_the_law(v, ctx.download(4).copy(), got, opt, "tiny128, rate behind counts")
    assert (got.bytes != first.bytes).any()
    _, _, _, rest = law.sections(got.bytes, 138, 4)
    assert rest.size == 5 * (2 * (got.layout.sci_stride - 4 * 138 * 138) + got.layout.dq_stride - 2 * 138 * 138) > 0 and not rest.any()
    assert want.sci[4].max() > 1.0


def test_the_padding_is_written_over_the_samples_of_another_layout():
    # A context of its own, calibrated twice: the slot's buffer first holds the payload of a 138^2 frame, then -- not
    # reallocated, it is large enough -- that of a 74^2 frame, whose padding falls where the first payload's samples lay.
    # (Within one mode the padding of every run falls on the same bytes, so a kernel that never wrote it would go unseen.)
    big, small = visit("tiny128"), visit("tiny")
    eng = engine.Engine(0, big.grism, big.detector, big.calibration, big.NSAMP, big.SAMPSEQ, big.SUBARRAY)
    try:
        ctx = eng.ctx
        gen = helpers.product_generator(big, 0)
        ctx.upload(4, gen.build_descriptor(eng, ima="counts", **big.frame_kwargs(0)))
        ctx.run_checked(4)
        first = ctx.ima(4)
        lay = ima.layout(74, small.NSAMP - 1)
        _, _, _, under = law.sections(first.bytes[:lay.nbytes], 74, small.NSAMP - 1)
        assert under.any() and np.count_nonzero(under) > under.size // 2        # samples lie where the padding will
        planes_small = small.calibration.for_mode(small.grism.name, small.SUBARRAY, small.SAMPSEQ,
                                                  np.asarray(small.read_times, dtype=float), detector=small.detector)
        ctx.set_calibration(planes_small["subarray"], planes_small["n_reads"], flat=planes_small.get("flat"),
                            pfl=planes_small.get("pfl"), sky=planes_small.get("sky"), lin=planes_small.get("lin"),
                            dark_sci=planes_small.get("dark_sci"), dark_err=planes_small.get("dark_err"),
                            zero_read=planes_small.get("zero_read"))
        opt = ima.Ima("rate")
        gen = helpers.product_generator(small, 0)
        ctx.upload(4, gen.build_descriptor(engine_of(small), ima=opt, **small.frame_kwargs(0)))
        ctx.run_checked(4)
        got = ctx.ima(4)
        assert got.layout == lay and got.bytes.size < first.bytes.size
        assert_is_the_law(small, ctx.download(4).copy(), got, opt, "tiny behind tiny128 in one buffer")
    finally:
        eng.close()


# ---- c. errors ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_slot_running_without_the_option():
    v = visit("tiny")
    eng = engine_of(v)
    ctx = eng.ctx
    L, hnd = ctx._L, ctx._h
    lay = ima.layout(eng.S, v.NSAMP - 1)
    buf = np.empty(lay.nbytes, dtype=np.uint8)
    out = buf.ctypes.data_as(C.c_void_p)
    ctx.upload(7, descriptor(v))
    ctx.run_checked(7)
    want = ctx.download(7).copy()
    assert L.wayne_exposure_download_ima(hnd, 7, out) == _lib.E_STATE              # without the option
    nan, inf = float("nan"), float("inf")
    for bad in ((3, 1, 20.0, 65000.0), (0, 1, 20.0, 65000.0), (7 | 8, 1, 20.0, 65000.0), (7 | 16, 2, 20.0, 65000.0),
                (7, 0, 20.0, 65000.0), (7, 3, 20.0, 65000.0), (7, -1, 20.0, 65000.0),
                (7, 1, 0.0, 65000.0), (7, 1, -1.0, 65000.0), (7, 2, nan, 65000.0), (7, 1, inf, 65000.0),
                (7, 1, 20.0, 0.0), (7, 2, 20.0, -1.0), (7, 1, 20.0, nan), (7, 1, 20.0, inf)):
        ctx.set_ima(7, True)
        assert ctx.has_ima(7)
        d = _lib.ImaDesc(*bad)
        assert L.wayne_exposure_set_ima(hnd, 7, C.byref(d)) == _lib.E_INVALID, bad
        assert L.wayne_exposure_download_ima(hnd, 7, out) == _lib.E_STATE, bad      # the refusal cleared the option
    ok = _lib.ImaDesc(7, 1, 20.0, 65000.0)
    for slot in (-1, 10000):
        assert L.wayne_exposure_set_ima(hnd, slot, C.byref(ok)) == _lib.E_INVALID
        assert L.wayne_exposure_download_ima(hnd, slot, out) == _lib.E_INVALID
    # a slot that is not uploaded
    assert L.wayne_exposure_set_ima(hnd, 200, C.byref(ok)) == _lib.E_STATE
    assert L.wayne_exposure_download_ima(hnd, 200, out) == _lib.E_STATE
    # the slot runs on, without the option
    ctx._slot_ima.pop(7, None)
    ctx.run_checked(7)
    np.testing.assert_array_equal(ctx.download(7), want)
    # the option still works on the slot afterwards: not before a run, then the law, then cleared by NULL and by an upload
    ctx.set_ima(7, "counts")
    assert L.wayne_exposure_download_ima(hnd, 7, out) == _lib.E_STATE              # set, but not run yet
    ctx.run_checked(7)
    got = ctx.ima(7)
    np.testing.assert_array_equal(ctx.download(7), want)
    assert_is_the_law(v, want, got, ima.Ima("counts"), "tiny after the refusals")
    assert L.wayne_exposure_download_ima(hnd, 7, out) == 0 and (buf == got.bytes).all()
    ctx.set_ima(7, None)
    assert not ctx.has_ima(7) and L.wayne_exposure_download_ima(hnd, 7, out) == _lib.E_STATE
    ctx.set_ima(7, True)
    ctx.upload(7, descriptor(v))
    assert not ctx.has_ima(7) and L.wayne_exposure_download_ima(hnd, 7, out) == _lib.E_STATE
    with pytest.raises(_lib.WayneError):
        ctx.ima(7)


# ---- d. the public path ---------------------------------------------------------------------------------------------
def test_scanning_frame_carries_the_calibrated_reads():
    v = visit("tiny128")
    opt = ima.Ima("counts", read_noise=15.0)
    frame = helpers.product_generator(v, 0).scanning_frame(ima=opt, **v.frame_kwargs(0))
    ctx = engine_of(v).ctx
    assert isinstance(frame.ima, ima.Payload) and frame.ima.ima is opt and frame.ima.bytes.dtype == np.uint8
    np.testing.assert_array_equal(frame.ima.bytes, ctx.ima(0).bytes)
    reads = np.stack([np.asarray(r) for r, _ in frame.reads])
    assert_is_the_law(v, reads, frame.ima, opt, "scanning_frame")
    plain = helpers.product_generator(v, 0).scanning_frame(**v.frame_kwargs(0))
    assert plain.ima is None
    for (a, _), (b, _) in zip(frame.reads, plain.reads):
        np.testing.assert_array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def file_equals_payload(path, payload, raw_path, units):
    hdus, raw = fitsio.read(path), fitsio.read(raw_path)
    n = payload.layout.R + 1
    assert len(hdus) == len(raw) == 1 + 5 * n and [h.name for h in hdus] == [h.name for h in raw]
    assert hdus[0].header["IMAUNIT"] == units.upper() and hdus[0].header["IMARN"] == 20.0 and hdus[0].header["IMASAT"] == 65000.0
    for key in raw[0].header.keys():
        if key not in ("DATE", "SIM-TIME", "COMMENT", "HISTORY", ""):
            assert hdus[0].header[key] == raw[0].header[key], key
    for r in range(n):
        at = 1 + 5 * (n - 1 - r)
        assert [h.name for h in hdus[at:at + 5]] == ["SCI", "ERR", "DQ", "SAMP", "TIME"]
        assert [h.header["BITPIX"] for h in hdus[at:at + 3]] == [-32, -32, 16]
        assert all(h.header["EXTVER"] == rh.header["EXTVER"] for h, rh in zip(hdus[at:at + 5], raw[at:at + 5]))
        for key in ("SAMPNUM", "SAMPTIME", "DELTATIM", "CRPIX1"):
            assert hdus[at].header[key] == raw[at].header[key], key
        assert (hdus[at].data.view(np.uint32) == payload.sci(r).view(np.uint32)).all()
        assert (hdus[at + 1].data.view(np.uint32) == payload.err(r).view(np.uint32)).all()
        assert (hdus[at + 2].data == payload.dq(r)).all()
        assert hdus[at + 3].header["PIXVALUE"] == (1 if r else 0) and hdus[at + 3].data is None and hdus[at + 4].data is None
        assert abs(hdus[at + 4].header["PIXVALUE"] - hdus[at].header["SAMPTIME"]) <= 1e-9        # t_k, the intervals summed
    return hdus


def test_the_visit_runner_delivers_the_payloads_and_writes_the_files(tmp_path):
    from wayne_amd import visit as wv
    v = visit("tiny128", n=3)
    seen = {}
    runner = wv.VisitRunner(v, 0, out_dir=str(tmp_path / "with"))
    kept = runner.run(range(3), keep=True, ima="counts", on_ima=lambda i, p: seen.__setitem__(i, p))
    assert sorted(seen) == sorted(runner.ima) == [0, 1, 2]
    plain_runner = wv.VisitRunner(v, 0, out_dir=str(tmp_path / "plain"))
    plain = plain_runner.run(range(3), keep=True)
    assert plain_runner.ima is None
    names = sorted(os.listdir(str(tmp_path / "with")))
    assert [m for m in names if m.endswith("_ima.fits")] == ["%04d_ima.fits" % (i + 1) for i in range(3)]
    assert not [m for m in os.listdir(str(tmp_path / "plain")) if m.endswith("_ima.fits")]
    for i in range(3):
        assert seen[i] is runner.ima[i]
        np.testing.assert_array_equal(kept[i].view(np.uint32), plain[i].view(np.uint32))
        assert_is_the_law(v, kept[i], seen[i], ima.Ima("counts"), "VisitRunner exposure %d" % i)
        file_equals_payload(str(tmp_path / "with" / ("%04d_ima.fits" % (i + 1))), seen[i],
                            str(tmp_path / "with" / ("%04d_raw.fits" % (i + 1))), "counts")
    assert (seen[0].bytes != seen[1].bytes).any()
    for m in (m for m in names if m.endswith("_raw.fits")):
        a = clock_free(open(str(tmp_path / "with" / m), "rb").read())
        b = clock_free(open(str(tmp_path / "plain" / m), "rb").read())
        assert a == b, m
    with pytest.raises(TypeError):
        wv.VisitRunner(v, 0).run(range(1), ima=3.0)
    with pytest.raises(ValueError):
        wv.VisitRunner(v, 0, out_dir=str(tmp_path / "refused"), device_fits=True).run(range(1), ima=True)


def test_the_cli_writes_ima_files_beside_the_raw_files(tmp_path):
    n = 3
    outs = {}
    for flag in ((), ("--ima",), ("--ima", "counts")):
        work = str(tmp_path / ("visit%d" % len(flag)))
        shutil.copytree(MINI, work)
        outs[flag] = run_visit.run(["-p", os.path.join(work, "params.yml"), "--max-exposures", str(n)] + list(flag))
    plain = outs[()]
    assert not [m for m in os.listdir(plain.outdir) if m.endswith("_ima.fits")]
    sums = {}
    for flag, units in ((("--ima",), "rate"), (("--ima", "counts"), "counts")):
        obs = outs[flag]
        names = sorted(m for m in os.listdir(obs.outdir) if m.endswith("_ima.fits"))
        assert names == ["%04d_ima.fits" % (i + 1) for i in range(n)]
        R = obs.NSAMP - 1
        for i, m in enumerate(names):
            raw_path = os.path.join(obs.outdir, "%04d_raw.fits" % (i + 1))
            hdus, raw = fitsio.read(os.path.join(obs.outdir, m)), fitsio.read(raw_path)
            assert len(hdus) == len(raw) == 1 + 5 * (R + 1) and [h.name for h in hdus] == [h.name for h in raw]
            assert hdus[0].header["IMAUNIT"] == units.upper() and hdus[0].data is None
            assert hdus[1].header["BUNIT"] == ("ELECTRONS/S" if units == "rate" else "ELECTRONS")
            last, zero = np.asarray(hdus[1].data), np.asarray(hdus[1 + 5 * R].data)
            assert last.dtype == np.dtype(">f4") and np.isfinite(last).all() and last.max() > 1.0 and not zero.any()
            assert (np.asarray(hdus[2].data)[5:-5, 5:-5] > 0).all() and not last[:5].any()
            assert hdus[3].header["BITPIX"] == 16 and hdus[4].header["PIXVALUE"] == 1 and hdus[4 + 5 * R].header["PIXVALUE"] == 0
            assert abs(hdus[5].header["PIXVALUE"] - raw[1].header["SAMPTIME"]) < 1e-9
            sums[(units, i)] = (last.astype(np.float64), hdus[5].header["PIXVALUE"])
            # the _raw files keep their bytes
            a = clock_free(open(raw_path, "rb").read())
            b = clock_free(open(os.path.join(plain.outdir, "%04d_raw.fits" % (i + 1)), "rb").read())
            assert a == b, m
    # the two units are the same electrons: the rate is the counts over the read's time, each rounded once to float32
    for i in range(n):
        rate, t = sums[("rate", i)]
        counts, _ = sums[("counts", i)]
        assert np.allclose(rate * t, counts, rtol=3e-7, atol=0.0)
    engine.close_all()


# ---- e. what an observer does with the file --------------------------------------------------------------------------
def test_differenced_reads_sum_to_the_devices_own_spectra():
    """On small256, the sky step and the rejection off: sum_y (SCI_{j+1} - SCI_j) of a counts-unit payload over the plan's
    window against the device's spectra_j[x], light-sensitive columns.  Both sum the same electrons; the payload holds them
    in float32, so the two differ by the storage alone: at most 2^-24 (|e_{j+1}| + |e_j|) a pixel (half an ulp each),
    summed over the window -- derived, no measured margin (the float64 sums themselves err 2^-29 of that)."""
    v = visit("small256")
    steps = extraction.ALL & ~extraction.SKY
    ctx = engine_of(v).ctx
    gen = helpers.product_generator(v, 0)
    ctx.upload(0, gen.build_descriptor(engine_of(v), extraction=extraction.ExtractionOptions(steps=steps), ima="counts",
                                       **v.frame_kwargs(0)))
    ctx.run_checked(0)
    reads = ctx.download(0).copy()
    spectra, _ = ctx.download_spectra(0)
    got = ctx.ima(0)
    plan = gen.extraction_plan
    R, S = v.NSAMP - 1, reads.shape[-1]
    e = law.restate(reads, planes(v), "counts").e
    worst = 0.0
    for j in range(R):
        lo, hi = int(plan.row_windows[j][0]), int(plan.row_windows[j][1])
        hi_plane = got.sci(j + 1)[lo:hi].astype(np.float64)
        lo_plane = got.sci(j)[lo:hi].astype(np.float64)
        total = (hi_plane - lo_plane).sum(axis=0)
        bound = 2.0 ** -24 * (np.abs(e[j + 1, lo:hi]) + np.abs(e[j, lo:hi])).sum(axis=0)
        err = np.abs(total - spectra[j])[5:-5]
        ratio = float((err / bound[5:-5]).max())
        worst = max(worst, ratio)
        print("interval %d, rows [%d, %d): worst |sum of differenced reads - spectra| = %.3g of the float32 bound" % (j, lo, hi, ratio))
        assert hi - lo >= 1 and np.abs(spectra[j][5:-5]).max() > 1e2
        assert (err <= bound[5:-5]).all(), (j, ratio)
    assert worst > 0.0                                     # (float32 storage is visible: the planes are not float64 in disguise)
