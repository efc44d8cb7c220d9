"""GPU: the noise-free expected image (wayne_exposure_set_expected, k_expect, --expected).

The law is tests/expected_law.py, built here from the slot's own debug_fetch counts and positions.  Tolerances:
  * device against law: |device - law| <= REL law + A_r per pixel of read interval r -- REL = extraction_law.REL (every
    term of E is >= 0, so the sum is its own magnitude), A_r = 2 Phi(-8) x (electrons of interval r): what the kernel's
    8 sigma cut may drop; the 5-pixel border is zero to the bit;
  * throwers against law: chi2/n = mean((acc_e - E)^2 / V) over the pixels with V >= 5 within 1 +- 5 sqrt(2 / n),
    n >= 1000 -- E the device's, V the law's; the law with the bins' sub-pixel fraction dropped must fall outside;
  * bytes: equal planes in any slot, on either stream, on a second run; reads and spectra bit-identical with the option.
CPU side (the law itself, host validation): tests/test_expected.py."""
import os
import shutil

import numpy as np
import pytest

import expected_law as law
import extraction_law
import helpers
from fits_words_law import clock_free
from wayne_amd import _lib, engine, fitsio, grism as wgrism, run_visit
from wayne_amd.tools import crop_central_box
from wayne_amd.sources import Contaminant

pytestmark = pytest.mark.gpu

REL = extraction_law.REL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI = os.path.join(ROOT, "tests", "fixtures", "mini_visit")
STARING = {"tiny": False, "tiny_g102": False, "tiny128": False, "small256": False, "stare256": True}
QUIET = dict(sky_background=0.0, cosmic_rate=None, add_dark=False, add_read_noise=False)


def prepare(name, rng_mode=_lib.RNG_SPLIT, E=None, **opts):
    """(visit, frame keywords, generator, engine, descriptor) of exposure 0 of a synthetic visit."""
    v = helpers.make_visit(name, **({"E": E} if E else {}))
    kw = v.frame_kwargs(0, **{k: opts.pop(k) for k in list(opts) if k in ("add_flat", "add_stellar_noise", "sky_background",
                                                                          "cosmic_rate", "add_dark", "add_read_noise")})
    pg = helpers.product_generator(v, 0)
    if STARING[name]:
        skw = {k: kw[k] for k in kw if k not in ("scan_speed", "sample_rate", "ssv_generator")}
        pg.prepare(staring=True, rng_mode=rng_mode, out_dtype=np.float32, **opts, **skw)
    else:
        pg.prepare(rng_mode=rng_mode, out_dtype=np.float32, **opts, **kw)
    eng, desc, _ = pg._prepared
    pg._prepared = None
    return v, kw, pg, eng, desc


def flat_function(v, eng, desc, x_ref, y_ref):
    """k -> f of sub-sample k for a source whose star is at (x_ref[k], y_ref[k]); None with the flat off."""
    if not (desc.flags & _lib.F_ADD_FLAT):
        return None
    N = eng.N
    cube = [np.asarray(crop_central_box(p, N), dtype=np.float32) for p in v.calibration.flat[v.grism.name]]
    wmin, wmax = v.calibration.flat_wl[v.grism.name]

    def f(k):
        m_t, _, m_w, c_w = wgrism.wavelength_calibration_coeffs(x_ref[k], y_ref[k], v.grism.trace_coeff, v.grism.wl_solution)
        return law.flat_of(cube, wmin, wmax, N, desc.sub_scale, (m_t, m_w, c_w), x_ref[k], y_ref[k])
    return f


def law_source(v, eng, desc, wl, counts, x, y, x_ref, y_ref, mode, lam=None, floor=False):
    ratio = v.grism.psf_ratio_poly(wl)
    n_h, n_l = law.split_counts(counts, ratio) if mode == "counts" else law.split_mean(lam, ratio)
    if floor:
        x, y = np.floor(x), np.floor(y)
    return dict(x=x, y=y, n_h=n_h, n_l=n_l, sig_h=v.grism.psf_sigmah_poly(wl), sig_l=v.grism.psf_sigmal_poly(wl),
                flat=flat_function(v, eng, desc, x_ref, y_ref))


def assert_parity(got, E, electrons_r, what=""):
    assert got.shape == E.shape and got.dtype == np.float64
    border = np.ones(got.shape[1:], dtype=bool)
    border[5:-5, 5:-5] = False
    assert not got[:, border].view(np.uint64).any(), what + ": the border is not zero to the bit"
    A = law.culling_bound(electrons_r)
    for r in range(got.shape[0]):
        err = np.abs(got[r] - E[r]) - (REL * E[r] + A[r])
        assert err.max() <= 0, "%s: read interval %d, pixel %s: device %r, law %r" % (
            what, r, np.unravel_index(err.argmax(), err.shape), got[r].flat[err.argmax()], E[r].flat[err.argmax()])


# ---- a. parity with the law, both modes -----------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [True, False], ids=["noise", "rounded"])
@pytest.mark.parametrize("flat", [True, False], ids=["flat", "noflat"])
@pytest.mark.parametrize("mode", ["counts", "mean"])
@pytest.mark.parametrize("name", list(STARING))
def test_the_device_renders_the_law(name, mode, flat, noise):
    v, kw, pg, eng, desc = prepare(name, add_flat=flat, add_stellar_noise=noise, expected=mode)
    ctx = eng.ctx
    slot = 2
    ctx.upload(slot, desc)
    assert ctx.has_expected(slot)
    ctx.run_checked(slot)
    got = ctx.expected(slot)
    counts, x, y, _ = ctx.debug_fetch(slot)
    h = pg._host_vectors
    lam, wl = helpers.reference_counts(v, kw, h["dur"])
    assert wl.size == desc.n_wl and counts.shape == lam.shape
    R = v.NSAMP - 1
    E, V = law.expected_image(eng.N, R, h["read"], [law_source(v, eng, desc, wl, counts, x, y, h["x_ref"], h["y_ref"], mode, lam)])
    thrown = counts.sum(axis=1) if mode == "counts" else np.maximum(lam, 0).sum(axis=1)
    electrons_r = np.bincount(h["read"], weights=thrown, minlength=R)
    assert_parity(got, E, electrons_r, "%s %s" % (name, mode))
    assert E.sum() > 0.05 * thrown.sum() > 0                    # (the comparison is not one of zeros; tiny's trace leaves its frame)
    if name == "tiny":
        # the 64 px frame: the wings cross the frame's edges, and frame row / column 0 would be hit
        inner = got[:, 5:-5, 5:-5]
        assert not inner[:, 0, :].any() and not inner[:, :, 0].any()
        assert inner[:, 1, :].any() and inner[:, :, 1].any() and inner[:, :, -1].any()
    if mode == "counts" and noise:
        # the counts the law used are the run's own draws, not the rounded means
        assert (counts != np.rint(lam)).any()


# ---- b. the throwers against the law ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rng", [_lib.RNG_SPLIT, _lib.RNG_PHILOX], ids=["split", "philox"])
@pytest.mark.parametrize("name", ["small256", "stare256"])
def test_the_throwers_scatter_about_the_expected_image(name, rng):
    v, kw, pg, eng, desc = prepare(name, rng_mode=rng, add_flat=False, expected="counts", **QUIET)
    ctx = eng.ctx
    slot = 1
    ctx.upload(slot, desc)
    ctx.run_front(slot)
    counts, x, y, acc = ctx.debug_fetch(slot, acc=True)
    ctx.run_back(slot)
    E = ctx.expected(slot)
    h = pg._host_vectors
    _, wl = helpers.reference_counts(v, kw, h["dur"])
    R = v.NSAMP - 1
    src = law_source(v, eng, desc, wl, counts, x, y, h["x_ref"], h["y_ref"], "counts")
    _, V = law.expected_image(eng.N, R, h["read"], [src])
    assert abs(acc.sum() - E.sum()) <= 6.0 * np.sqrt(max(counts.sum() - E.sum(), 1.0)) + 1.0
    chi2, n = law.chi2_per_pixel(acc, E, V)
    band = 5.0 * np.sqrt(2.0 / max(n, 1))
    print("%s rng %d: chi2/n = %.4f over n = %d pixels with V >= 5 (band +- %.3f)" % (name, rng, chi2, n, band))
    assert n >= 1000
    assert abs(chi2 - 1.0) <= band, (chi2, n)
    E0, V0 = law.expected_image(eng.N, R, h["read"], [law_source(v, eng, desc, wl, counts, x, y, h["x_ref"], h["y_ref"],
                                                                 "counts", floor=True)])
    chi2_0, n0 = law.chi2_per_pixel(acc, E0, V0)
    print("%s rng %d, fraction dropped: chi2/n = %.3f over n = %d" % (name, rng, chi2_0, n0))
    assert n0 >= 1000 and abs(chi2_0 - 1.0) > 5.0 * np.sqrt(2.0 / n0)


# ---- c. contaminants ------------------------------------------------------------------------------------------------
def single(pg, desc, c, expected):
    """The single-source exposure of contaminant c (tests/test_contaminants_gpu.py): offset positions, its spectrum, no
    depth, the derived seed."""
    h = pg._host_vectors
    return _lib.make_desc(_lib.source_seed(desc.seed, c.tag), desc.exposure_index, desc.flags, desc.sub_scale, c.wl, c.flux,
                          None, h["x_ref"] + c.dx, h["y_ref"] + c.dy, h["dur"], h["read"], pg._read_dt, replay_seed=h["seeds"],
                          rng_mode=desc.rng_mode, threads_compat=desc.threads_compat, sky_ct_s=desc.sky_ct_s,
                          cosmic_rate=-1.0, scale_factor=desc.scale_factor, noise_mean=desc.noise_mean,
                          noise_std=desc.noise_std, expected=expected)


@pytest.mark.parametrize("mode", ["counts", "mean"])
def test_sources_add_up(mode):
    v, kw, pg, eng, desc = prepare("small256", expected=mode)
    ctx = eng.ctx
    wl, fl = desc._keep[0], desc._keep[1]
    c1 = Contaminant(25.0, -30.0, wl.copy(), fl * 0.5, 1)
    # half off the frame: the trace starts ~40 px right of the star and is ~150 px long
    c2 = Contaminant(95.0, 12.0, wl.copy(), fl * 0.3 * (1.0 + (wl - wl.mean())), 2)

    def run(d, sources=None):
        ctx.upload(3, d)
        if sources is not None:
            ctx.set_sources(3, sources)
            ctx.set_expected(3, mode)            # (in either order with the sources)
        ctx.run_checked(3)
        return ctx.expected(3)

    e_t, e_1, e_2 = run(desc), run(single(pg, desc, c1, mode)), run(single(pg, desc, c2, mode))
    e_all = run(desc, [c1, c2])
    assert e_1.sum() > 1e4 and e_2.sum() > 1e4
    x2 = ctx.debug_fetch_source(3, 2)[1]
    assert (x2 < eng.N).any() and (x2 > eng.N + 20).any()           # c2 is half off the frame
    assert e_2.sum() < 0.8 * 0.3 / 0.5 * e_1.sum()
    want = e_t + e_1 + e_2
    np.testing.assert_allclose(e_all, want, rtol=REL, atol=0)


# ---- d. bytes -------------------------------------------------------------------------------------------------------
def test_the_same_bytes_everywhere_and_nothing_else_changes():
    v, kw, pg, eng, desc = prepare("small256", expected="counts", extraction=True)
    _, _, _, _, plain = prepare("small256", extraction=True)
    ctx = eng.ctx

    def run(slot, d):
        ctx.upload(slot, d)
        ctx.run_checked(slot)
        return ctx.download(slot).copy(), [a.copy() for a in ctx.download_spectra(slot)]

    reads0, spectra0 = run(0, desc)
    e0 = ctx.expected(0)
    assert e0.sum() > 1e6
    ctx.run_checked(0)                                   # a second run of the same upload
    np.testing.assert_array_equal(ctx.expected(0).view(np.uint64), e0.view(np.uint64))
    reads5, _ = run(5, desc)                             # another slot, the other stream
    np.testing.assert_array_equal(ctx.expected(5).view(np.uint64), e0.view(np.uint64))
    # an upload without the option: no plane any more, and reads and spectra as with it
    reads_p, spectra_p = run(0, plain)
    assert not ctx.has_expected(0)
    with pytest.raises(_lib.WayneError) as e:
        ctx.expected(0)
    assert e.value.status == _lib.E_STATE
    np.testing.assert_array_equal(reads_p.view(np.uint32), reads0.view(np.uint32))
    np.testing.assert_array_equal(reads5.view(np.uint32), reads0.view(np.uint32))
    for a, b in zip(spectra_p, spectra0):
        np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))
    # ... and with it again: the plane it had
    run(0, desc)
    np.testing.assert_array_equal(ctx.expected(0).view(np.uint64), e0.view(np.uint64))
    # a run the library repeats (status bit 1: a bin beyond the lanes' reach) renders again
    _lib.set_knob_all("lane_reach", "5")
    try:
        n0 = ctx.reruns
        ctx.upload(4, desc)
        ctx.run(4)
        again = ctx.expected(4)
        assert ctx.reruns == n0 + 1
        np.testing.assert_array_equal(again.view(np.uint64), e0.view(np.uint64))
    finally:
        _lib.set_knob_all("lane_reach", None)


# ---- e. errors ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_slot_usable():
    v, kw, pg, eng, desc = prepare("tiny")
    ctx = eng.ctx
    L, hnd = ctx._L, ctx._h
    ctx.upload(7, desc)
    ctx.run_checked(7)
    want = ctx.download(7).copy()
    # download without the option
    out = np.empty((v.NSAMP - 1, eng.S, eng.S))
    assert L.wayne_exposure_download_expected(hnd, 7, _lib.ptr(out, _lib.C.c_double)) == _lib.E_STATE
    # a bad mode
    for bad in (3, -1):
        assert L.wayne_exposure_set_expected(hnd, 7, bad) == _lib.E_INVALID
    assert not ctx.has_expected(7)
    # a slot that is not uploaded
    assert L.wayne_exposure_set_expected(hnd, 200, 1) == _lib.E_STATE
    assert L.wayne_exposure_download_expected(hnd, 200, _lib.ptr(out, _lib.C.c_double)) == _lib.E_STATE
    ctx.run_checked(7)
    np.testing.assert_array_equal(ctx.download(7), want)
    # replay mode
    _, _, _, _, replay = prepare("tiny", rng_mode=_lib.RNG_REPLAY)
    ctx.upload(7, replay)
    assert L.wayne_exposure_set_expected(hnd, 7, 1) == _lib.E_INVALID
    with pytest.raises(_lib.WayneError):
        ctx.set_expected(7, "counts")
    assert not ctx.has_expected(7)
    ctx.run_checked(7)
    assert np.isfinite(ctx.download(7)).all()
    # ... and the option still works on the slot afterwards, and clears
    ctx.upload(7, desc)
    ctx.set_expected(7, "mean")
    ctx.run_checked(7)
    assert ctx.expected(7).sum() > 1e3
    np.testing.assert_array_equal(ctx.download(7), want)
    ctx.set_expected(7, None)
    assert not ctx.has_expected(7)


# ---- f. the public path ---------------------------------------------------------------------------------------------
def test_scanning_frame_carries_the_expected_image():
    v = helpers.make_visit("tiny128")
    pg = helpers.product_generator(v, 0)
    frame = pg.scanning_frame(expected="counts", **v.frame_kwargs(0))
    ctx = engine.get_engine(0, v.grism, v.detector, v.calibration, v.NSAMP, v.SAMPSEQ, v.SUBARRAY).ctx
    S = v.detector.full_size(v.SUBARRAY)
    assert frame.expected.shape == (v.NSAMP - 1, S, S) and frame.expected.dtype == np.float64
    np.testing.assert_array_equal(frame.expected.view(np.uint64), ctx.expected(0).view(np.uint64))
    assert frame.expected.sum() > 0.2 * v.E
    plain = helpers.product_generator(v, 0).scanning_frame(**v.frame_kwargs(0))
    assert plain.expected is None
    for (a, _), (b, _) in zip(frame.reads, plain.reads):
        np.testing.assert_array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def test_the_visit_runner_delivers_the_planes():
    from wayne_amd import visit as wv
    v = helpers.make_visit("tiny128", n_exposures=3)
    seen = {}
    runner = wv.VisitRunner(v, 0)
    kept = runner.run(range(3), keep=True, expected="mean", on_expected=lambda i, e: seen.__setitem__(i, e))
    assert sorted(seen) == sorted(runner.expected) == [0, 1, 2]
    plain = wv.VisitRunner(v, 0).run(range(3), keep=True)
    for i in range(3):
        np.testing.assert_array_equal(seen[i], runner.expected[i])
        assert seen[i].sum() > 0.2 * v.E and (i == 0 or (seen[i] != seen[0]).any())
        np.testing.assert_array_equal(kept[i].view(np.uint32), plain[i].view(np.uint32))


def test_the_cli_writes_exp_files_beside_the_raw_files(tmp_path, monkeypatch):
    from wayne_amd import expected as wexp
    n = 6
    outs = {}
    delivered = {}
    write = wexp.write_fits

    def recording(path, exposure, planes, mode):
        delivered[os.path.basename(path)] = np.array(planes)        # what the context delivered for the file
        return write(path, exposure, planes, mode)
    monkeypatch.setattr(wexp, "write_fits", recording)
    for flag in ((), ("--expected", "counts")):
        work = str(tmp_path / ("visit%d" % len(flag)))
        shutil.copytree(MINI, work)
        obs = run_visit.run(["-p", os.path.join(work, "params.yml"), "--max-exposures", str(n)] + list(flag))
        outs[flag] = obs
    plain, obs = outs[()], outs[("--expected", "counts")]
    names = sorted(m for m in os.listdir(obs.outdir) if m.endswith("_exp.fits"))
    assert names == ["%04d_exp.fits" % (i + 1) for i in range(n)]
    assert not [m for m in os.listdir(plain.outdir) if m.endswith("_exp.fits")]
    assert sorted(delivered) == names
    for i, m in enumerate(names):
        hdus = fitsio.read(os.path.join(obs.outdir, m))
        raw = fitsio.read(os.path.join(obs.outdir, "%04d_raw.fits" % (i + 1)))
        assert hdus[0].header["EXPMODE"] == "counts" and hdus[0].data is None
        for key in raw[0].header.keys():
            if key not in ("DATE", "SIM-TIME", "COMMENT", "HISTORY", ""):
                assert hdus[0].header[key] == raw[0].header[key], key
        R = obs.NSAMP - 1
        assert [h.name for h in hdus[1:]] == ["EXPECT"] * R
        assert [h.header["EXTVER"] for h in hdus[1:]] == list(range(1, R + 1))
        assert all(h.header["BITPIX"] == -64 for h in hdus[1:])
        planes = np.array([np.asarray(h.data, dtype=np.float64) for h in hdus[1:]])
        assert planes.sum() > 0 and not planes[:, :5, :].any()
        np.testing.assert_array_equal(planes.view(np.uint64), delivered[m].view(np.uint64))
        # the _raw files keep their bytes
        a = clock_free(open(os.path.join(obs.outdir, "%04d_raw.fits" % (i + 1)), "rb").read())
        b = clock_free(open(os.path.join(plain.outdir, "%04d_raw.fits" % (i + 1)), "rb").read())
        assert a == b, m
    engine.close_all()
