"""GPU: star spots in the device light curves (wayne_exposure_set_spots, k_lightcurve_spots).

Everything runs on `small256` with K = 9.  With rp0 the mean radius ratio, the planet's track makes the nine rows
  0 out of transit; 1 in transit far from every spot; 2 external tangency with spot A, d = (rp0 + r)(1 - 1e-4);
  3 a generic partial overlap with A, the star's centre off the lens axis; 4 t* beyond A's centre (d = 0.04 < sqrt(p^2 -
  r^2)); 5 internal tangency with the large spot B, d = (r - rp0)(1 -+ 1e-4) -- K is the visit's, so the two signs are two
  tracks, "minus" and "plus"; 6 the planet wholly inside B (r = 0.2); 7 the small spot C (r = 0.05) wholly inside the
  planet; 8 behind the star, hidden > 0, where it would cross B.
The radius ratio varies by 0.2 % over the wavelengths, so at the tangencies some columns lie on either side of the case
boundary.  Spots: A with a temperature (4200 K on 5000 K), B with contrast 0.7, C a facula with contrast 1.1; the case
"eight" adds five more, one of them crossed on row 1.  Coefficients: the single set, and the table of
tests/test_ld_table_gpu.py.  Bounds:
  * the kernel alone (debug_depth of the spotted run against spots.apply of debug_depth of the unspotted run of the same
    slot): 256 * 2^-52 * (|depth| F0 + sum_i |1 - c| (Q_0 + S_0)) / (F0 - D), formed from the law's own terms -- the rule's
    200 non-negative terms summed recursively, a dozen roundings and a few units of sin / cos / acos each (the bound of
    the C ABI in tests/test_spots.py, carried through the law); equality on rows 0 and 8 and on unsized columns;
  * end to end (debug_depth against DeviceDepths.host_matrix()): 2e-8 * F0 / (F0 - D), the light-curve kernels' own bound
    (tests/test_lightcurve.py) carried through the rescale;
  * frames: the two bounds of tests/test_ld_table_gpu.py (max < 0.5, median < 1e-6);
  * bytes: equal where nothing may move.
CPU side (the rule, the law, configuration, header): tests/test_spots.py."""
import ctypes as C
import os
import shutil
import types

import numpy as np
import pytest
import yaml

import helpers
from fits_words_law import clock_free
from wayne_amd import _lib, engine, fitsio, lightcurve as lc, run_visit, spots, tools

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI = os.path.join(ROOT, "tests", "fixtures", "mini_visit")
LD = [0.800627, -0.757066, 0.897268, -0.384804]
ULP = 256 * 2.0 ** -52
ATOL = 2e-8

A = (-0.3, 0.35, 0.10)
B = (0.35, -0.3, 0.20)
SMALL = (0.1, 0.6, 0.05)
MORE = [(-0.65, -0.4, 0.05), (0.7, 0.3, 0.06), (0.0, -0.7, 0.08), (-0.1, 0.0, 0.07), (0.6, 0.6, 0.05)]
MORE_CONTRAST = [0.5, 1.3, 0.0, 0.9, 1.0]


def table_at(wl):
    s = np.clip((np.asarray(wl, dtype=float) - 1.1) / 0.6, 0.0, 1.0)
    return np.stack([0.55 + 0.25 * s, -0.2 - 0.55 * s, 0.5 + 0.4 * s, -0.25 - 0.13 * s], axis=1)


class Case(object):
    """The visit, its engine and the inputs of the parity cases; device matrices are computed once and kept."""

    def __init__(self):
        v = self.v = helpers.make_visit("small256")
        self.kw = v.frame_kwargs(0)
        self.pg = helpers.product_generator(v, 0)
        self.eng = engine.get_engine(0, v.grism, v.detector, v.calibration, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)
        self.i0, self.i1 = tools.crop_spectrum_ind(v.grism.wl_limits[0], v.grism.wl_limits[1], v.wl)
        K = len(v.sample_mid_points)
        assert K == 9
        rp0 = float(np.sqrt(v.depth0.mean()))
        self.spec = v.depth0 * (1 + 0.004 * np.sin(np.arange(v.depth0.size) / 300.0))
        self.spec[self.i0 + 7] = -1.0                         # a column without a radius ratio
        self.tracks = {}
        for name, sign in (("minus", -1.0), ("plus", 1.0)):
            d_ext = (rp0 + A[2]) * (1 - 1e-4)
            d_int = (B[2] - rp0) * (1 + sign * 1e-4)
            P = np.array([(1.5, 0.3), (-0.6, -0.5), (A[0] + 0.6 * d_ext, A[1] - 0.8 * d_ext),
                          (A[0] - 0.8 * 0.15, A[1] + 0.6 * 0.15), (A[0], A[1] + 0.04), (B[0] + d_int, B[1]),
                          (B[0], B[1] + 0.03), (SMALL[0] + 0.02, SMALL[1]), (B[0] + 0.1, B[1])])
            z = np.hypot(P[:, 0], P[:, 1])
            hidden = np.zeros(K)
            z[8] += 10.0
            hidden[8] = 0.6
            self.tracks[name] = (P[:, 0].copy(), P[:, 1].copy(), z, hidden)
        three = spots.StarSpots([spots.Spot(A[0], A[1], A[2], temperature=4200.0), spots.Spot(B[0], B[1], B[2], contrast=0.7),
                                 spots.Spot(SMALL[0], SMALL[1], SMALL[2], contrast=1.1)], photosphere_temperature=5000.0)
        eight = spots.StarSpots(list(three.spots) + [spots.Spot(x, y, r, contrast=c) for (x, y, r), c in
                                                     zip(MORE, MORE_CONTRAST)], photosphere_temperature=5000.0)
        self.star = {"three": three, "eight": eight}
        self.table = table_at(v.wl)
        self._got = {}

    def depths(self, track="minus", ld="single", star="three"):
        X, Y, z, hidden = self.tracks[track]
        geo = None if star is None else self.star[star].geometry(X, Y, self.v.wl)
        return lc.DeviceDepths(z, hidden, self.spec, LD if ld == "single" else self.table, spots=geo)

    def device_matrix(self, dd, slot=0, ctx=None, runs=1):
        ctx = ctx or self.eng.ctx
        ctx.upload(slot, self.pg.build_descriptor(self.eng, **dict(self.kw, planet_signal=dd)))
        for _ in range(runs):
            ctx.run_front(slot)
            got = ctx.debug_depth(slot)
            ctx.run_back(slot)
        return got

    def got(self, track, ld, star):
        key = (track, ld, star)
        if key not in self._got:
            self._got[key] = self.device_matrix(self.depths(track, ld, star))
        return self._got[key]


@pytest.fixture(scope="module")
def case(gpu_ctx):
    return Case()


CASES = [("minus", "single", "three"), ("plus", "single", "three"), ("minus", "table", "three"), ("plus", "table", "three"),
         ("minus", "table", "eight")]


@pytest.mark.parametrize("track,ld,star", CASES)
def test_kernel_alone(case, track, ld, star):
    """Worst |device - law| seen on the MI355X: 5.2e-18, 0.002 of the bound, in each of the five cases."""
    i0, i1 = case.i0, case.i1
    dd = case.depths(track, ld, star)
    plain = case.got(track, ld, None)
    got = case.got(track, ld, star)
    geo = dd.spots.crop(i0, i1)
    coeffs = LD if ld == "single" else case.table[i0:i1]
    parts = {}
    want = geo.apply(plain, dd.z_tr, dd.hidden, case.spec[i0:i1], coeffs, parts=parts)
    F0, D = parts["F0"], parts["D"]
    bound = ULP * (np.abs(plain) * F0 + parts["mag"]) / (F0 - D)
    err = np.abs(got - want)
    print("k_lightcurve_spots %s/%s/%s: worst |device - law| / bound = %.3f (max |device - law| = %.3e)" % (
        track, ld, star, (err[bound > 0] / bound[bound > 0]).max(), err.max()))
    assert np.all(err <= bound)
    for k in (0, 8):
        assert got[k].tobytes() == plain[k].tobytes()
    assert np.all(got[0] == 0.0) and np.all(got[:, 7] == 0.0) and got[:, 7].tobytes() == plain[:, 7].tobytes()
    # the rows do what they were chosen for
    p = np.sqrt(np.where(case.spec[i0:i1] >= 0, case.spec[i0:i1], np.nan))
    sized = np.isfinite(p)
    X, Y = dd.spots.X, dd.spots.Y
    d_ext = np.hypot(X[2] - A[0], Y[2] - A[1])
    assert np.any(d_ext < p[sized] + A[2]) and np.any(d_ext >= p[sized] + A[2])        # both sides of the tangency
    d_int = np.hypot(X[5] - B[0], Y[5] - B[1])
    assert np.any(d_int <= B[2] - p[sized]) and np.any(d_int > B[2] - p[sized])
    with np.errstate(invalid="ignore"):                     # (row 0: 0 / 0)
        ratio = got[:, sized] / plain[:, sized]
    scale = (F0 / (F0 - D))[sized]
    if star == "three":
        np.testing.assert_allclose(ratio[1], scale, rtol=1e-12)                        # unocculted: the rescale alone
    else:
        assert np.all(ratio[1] < scale * (1 - 1e-4))                                   # (a dark spot crossed on row 1)
    assert np.all(ratio[3] < scale) and np.all(ratio[4] < scale) and np.all(ratio[6] < scale)   # dark spots crossed
    assert np.all(ratio[7] > scale)                                                    # the facula crossed


@pytest.mark.parametrize("track,ld,star", CASES)
def test_end_to_end(case, track, ld, star):
    """Worst |device - host_matrix| seen on the MI355X: 3.8e-9, 3.7e-9, 3.9e-9, 3.7e-9, 4.0e-9 (the cases in order)."""
    i0, i1 = case.i0, case.i1
    dd = case.depths(track, ld, star)
    got = case.got(track, ld, star)
    want = dd.host_matrix()[:, i0:i1]
    f0, D = spots.unocculted_deficit(LD if ld == "single" else case.table[i0:i1], dd.spots.cx, dd.spots.cy,
                                     dd.spots.radius, dd.spots.contrast[:, i0:i1])
    print("spots %s/%s/%s: max |device - host_matrix| = %.3e" % (track, ld, star, np.abs(got - want).max()))
    assert np.all(np.abs(got - want) <= ATOL * (f0 / (f0 - D))[None, :])
    assert np.abs(got - case.got(track, ld, None)).max() > 1e-4


def test_frames_equal_host_matrix(case):
    # replay thrower, noise sources off: the exposure built from the device's matrix equals the one given host_matrix()
    dd = case.depths("minus", "table", "three")
    off = dict(add_stellar_noise=False, sky_background=0.0, cosmic_rate=None, add_dark=False, add_read_noise=False)

    def frames(signal):
        return np.stack([r[0] for r in case.pg.scanning_frame(rng_mode=_lib.RNG_REPLAY, out_dtype=np.float64,
                                                              **dict(case.kw, planet_signal=signal, **off)).reads])
    a, b = frames(dd), frames(dd.host_matrix())
    c = frames(case.depths("minus", "table", None))           # ... and differs from the unspotted exposure
    assert np.abs(a - b).max() < 0.5
    assert np.median(np.abs(a - b)) < 1e-6
    assert np.abs(a - c).max() > 0.5


def test_nothing_else_moved(case):
    v = case.v
    fresh = engine.Engine(0, v.grism, v.detector, v.calibration, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)
    try:
        ctx = fresh.ctx
        for ld in ("single", "table"):
            plain, spotted = case.depths("minus", ld, None), case.depths("minus", ld, "three")
            before = case.device_matrix(plain, ctx=ctx)                # no spots were ever set on this context (first pass)
            with_spots = case.device_matrix(spotted, ctx=ctx)
            after = case.device_matrix(plain, ctx=ctx)                 # set -> re-upload without
            assert before.tobytes() == after.tobytes() == case.got("minus", ld, None).tobytes()
            assert before.tobytes() != with_spots.tobytes()
            # set -> cleared on the same upload
            ctx.upload(0, case.pg.build_descriptor(fresh, **dict(case.kw, planet_signal=spotted)))
            ctx.set_spots(0, None)
            ctx.run_front(0)
            cleared = ctx.debug_depth(0)
            ctx.run_back(0)
            assert cleared.tobytes() == before.tobytes()
            # the same bytes in slots 0 and 5 (the two streams), on a second run, and in another context
            assert with_spots.tobytes() == case.got("minus", ld, "three").tobytes()
            assert case.device_matrix(spotted, slot=5, ctx=ctx).tobytes() == with_spots.tobytes()
            assert case.device_matrix(spotted, slot=5, ctx=ctx, runs=2).tobytes() == with_spots.tobytes()
        ctx.synchronize()
    finally:
        fresh.close()


def test_refusals(case):
    ctx, i0, i1 = case.eng.ctx, case.i0, case.i1
    plain = case.depths("minus", "single", None)
    good = case.depths("minus", "single", "three").spots.crop(i0, i1)
    want = case.device_matrix(plain, slot=2)
    W, K = i1 - i0, 9

    def geometry(**change):
        g = types.SimpleNamespace(n=good.n, cx=good.cx.copy(), cy=good.cy.copy(), radius=good.radius.copy(),
                                  contrast=good.contrast.copy(), X=good.X.copy(), Y=good.Y.copy())
        for k, val in change.items():
            setattr(g, k, val)
        return g

    def refused(status, g, slot=2):
        with pytest.raises(_lib.WayneError) as e:
            ctx.set_spots(slot, g)
        assert e.value.status == status

    refused(_lib.E_STATE, good, slot=201)                      # a slot that is not uploaded

    def entry(arr, i, val):
        out = arr.copy()
        out.reshape(-1)[i] = val
        return out

    nan_track = entry(good.X, 3, np.nan)
    bad = [geometry(radius=entry(good.radius, 1, 0.0)), geometry(radius=entry(good.radius, 1, np.inf)),
           geometry(radius=entry(good.radius, 1, np.nan)), geometry(cx=entry(good.cx, 0, -0.9)),          # beyond 0.98
           geometry(cx=entry(good.cx, 2, A[0] + 0.1), cy=entry(good.cy, 2, A[1])),                        # overlapping
           geometry(contrast=entry(good.contrast, W + 5, -0.1)), geometry(contrast=entry(good.contrast, 5, np.nan)),
           geometry(contrast=good.contrast[:, :-1]), geometry(X=good.X[:-1], Y=good.Y[:-1]),              # W, K
           geometry(X=nan_track)]
    for g in bad:
        ctx.set_spots(2, good)                                 # spots are set, then refused ones: the slot runs unspotted
        refused(_lib.E_INVALID, g)
        ctx.run_front(2)
        got = ctx.debug_depth(2)
        ctx.run_back(2)
        assert got.tobytes() == want.tobytes()
    # a track that is not finite on the row behind the star is not a defect
    ctx.set_spots(2, geometry(X=entry(good.X, 8, np.nan)))
    ctx.run_front(2)
    got = ctx.debug_depth(2)
    ctx.run_back(2)
    assert got.tobytes() == case.got("minus", "single", "three").tobytes()
    # more than 8 spots: through the C symbol itself (the Python wrapper refuses first)
    with pytest.raises(ValueError):
        ctx.set_spots(2, geometry(n=9))
    desc = _lib.SpotsDesc()
    desc.n = 9
    c_, x_, y_ = _lib.f64(np.ones((9, W))), _lib.f64(good.X), _lib.f64(good.Y)
    desc.contrast, desc.px, desc.py = (_lib.ptr(a, C.c_double) for a in (c_, x_, y_))
    assert ctx._L.wayne_exposure_set_spots(ctx._h, 2, C.byref(desc), W, K) == _lib.E_INVALID
    # F0 - D <= 0: limb darkening whose disc flux the spots use up
    dark = lc.DeviceDepths(plain.z_tr, plain.hidden, plain.planet_spectrum, [4.9, 0.0, 0.0, 0.0])
    ctx.upload(2, case.pg.build_descriptor(case.eng, **dict(case.kw, planet_signal=dark)))
    big = geometry(n=1, cx=np.zeros(1), cy=np.zeros(1), radius=np.full(1, 0.9), contrast=np.zeros((1, W)))
    refused(_lib.E_INVALID, big)
    ctx.run(2)
    # a slot whose depth matrix was uploaded has no device light curve
    ctx.upload(2, case.pg.build_descriptor(case.eng, **dict(case.kw, planet_signal=plain.host_matrix())))
    refused(_lib.E_INVALID, good)
    ctx.set_spots(2, None)                                     # clearing is never refused
    ctx.run_front(2)
    got = ctx.debug_depth(2)
    ctx.run_back(2)
    np.testing.assert_array_equal(got, plain.host_matrix()[:, i0:i1])
    ctx.synchronize()


def _section(obs_plain):
    """Two spots for the mini visit: one unocculted, one the planet reaches in exposure 2 (ingress)."""
    return {"photosphere_temperature": 5000, "list": [{"x": -0.21, "y": 0.33, "radius": 0.10, "temperature": 4200},
                                                      {"at_phase": -0.0125, "radius": 0.12, "contrast": 0.75}]}


def _write_params(work, section):
    with open(os.path.join(MINI, "params.yml")) as f:
        cfg = yaml.safe_load(f)
    if section is not None:
        cfg["target"]["spots"] = section
    with open(os.path.join(work, "params.yml"), "w") as f:
        yaml.safe_dump(cfg, f)


def test_run_visit_with_spots(case, tmp_path):
    work = str(tmp_path / "visit")
    shutil.copytree(MINI, work)
    params = os.path.join(work, "params.yml")
    section = _section(None)
    _write_params(work, None)
    plain = run_visit.run(["-p", params, "--max-exposures", "2"])
    names = ["%04d_raw.fits" % n for n in (1, 2)]

    def file_bytes(obs):
        out = []
        for name in names:
            with open(os.path.join(obs.outdir, name), "rb") as f:
                out.append(clock_free(f.read()))               # (DATE and SIM-TIME blanked)
        return out

    plain_bytes = file_bytes(plain)
    assert all("SPOTS" not in fitsio.scan(os.path.join(plain.outdir, n))[0][0] for n in names)
    _write_params(work, section)
    obs = run_visit.run(["-p", params, "--max-exposures", "2", "--resume"])      # the section was added: regenerated
    star = obs.spots
    for n in (1, 2):
        hdr = fitsio.scan(os.path.join(obs.outdir, "%04d_raw.fits" % n))[0][0]
        assert hdr["SPOTS"] is True and hdr["NSPOTS"] == 2 and hdr["SPTHASH"].strip() == star.hash(obs.wl)
        assert (hdr["SPTX1"], hdr["SPTY1"], hdr["SPTR1"], hdr["SPTR2"], hdr["SPTC2"]) == (-0.21, 0.33, 0.10, 0.12, 0.75)
        assert obs.exposure_file_is_whole(n)
    spotted_bytes = file_bytes(obs)
    assert spotted_bytes[0] != plain_bytes[0]
    # Observation.generate_lightcurves is the device's matrix: exposure 2 (the planet reaches the second spot), by hand
    gen = obs._generate_exposure(obs.exp_start_times[1], 2, prepare_only=True)
    eng, desc, _ = gen._prepared
    gen._prepared = None
    _, mid, _, _ = gen._gen_scanning_sample_times(obs.sample_rate)
    t = obs.exp_start_times[1] + mid / (86400. * 1000.)
    dd = obs.device_depths(t)
    assert dd.spots.contrast.shape == (2, obs.wl.size) and desc._spots is not None
    eng.ctx.upload(0, desc)
    eng.ctx.run_front(0)
    got = eng.ctx.debug_depth(0)
    eng.ctx.run_back(0)
    eng.ctx.synchronize()
    i0, i1 = tools.crop_spectrum_ind(obs.grism.wl_limits[0], obs.grism.wl_limits[1], obs.wl)
    want = 1.0 - obs.generate_lightcurves(t)[:, i0:i1]
    f0, D = spots.unocculted_deficit(LD, star.cx, star.cy, star.radius, star.on_grid(obs.wl)[:, i0:i1])
    print("run_visit: max |device - generate_lightcurves| = %.3e" % np.abs(got - want).max())
    assert np.all(np.abs(got - want) <= ATOL * (f0 / (f0 - D))[None, :] + 2.0 ** -52)      # (1 - (1 - x): one rounding)
    assert want.max() > 1e-3
    crossing = np.hypot(dd.spots.X - star.cx[1], dd.spots.Y - star.cy[1]) < np.sqrt(obs.planet_spectrum.max()) + 0.12
    assert crossing.any()                                      # the second spot is reached within the exposure
    # --resume: a spot changed, a spot removed, the section removed -- regenerated each time; unchanged: kept
    stamp = [os.path.getmtime(os.path.join(obs.outdir, n)) for n in names]
    kept = run_visit.run(["-p", params, "--max-exposures", "2", "--resume"])
    assert [os.path.getmtime(os.path.join(kept.outdir, n)) for n in names] == stamp and file_bytes(kept) == spotted_bytes
    changed = dict(section, list=[section["list"][0], dict(section["list"][1], contrast=0.7)])
    removed = dict(section, list=section["list"][:1])
    seen = [spotted_bytes[1]]
    for sec in (changed, removed):
        _write_params(work, sec)
        again = run_visit.run(["-p", params, "--max-exposures", "2", "--resume"])
        now = file_bytes(again)
        assert now[1] not in seen
        seen.append(now[1])
    _write_params(work, None)
    back = run_visit.run(["-p", params, "--max-exposures", "2", "--resume"])
    assert file_bytes(back) == plain_bytes                     # without the section the files keep their bytes
