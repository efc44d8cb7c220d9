"""GPU: limb darkening per wavelength bin on the device (wayne_exposure_set_limb_darkening, k_lightcurve_ld).

Everything runs on `small256` with K = 9 and the z vector of test_lightcurve.test_device_depths_interpolated_in_radius_ratio
(no transit, both contacts +- 1e-4 rp, the limb, 0.6, rp 1.0002, rp 0.3, 0): the interpolated and the per-wavelength path
both run.  The table is the issue's, s = clip((wl - 1.1) / 0.6, 0, 1), a = (0.55 + 0.25 s, -0.2 - 0.55 s, 0.5 + 0.4 s,
-0.25 - 0.13 s).  Bounds:
  * debug_depth against the numpy law (every wavelength) and against oracle/lc_oracle.c called once per wavelength with
    that wavelength's coefficients (every 8th): atol 2e-8, the bound tests/test_lightcurve.py gives k_lightcurve for its
    float32 integrand -- the method is the same (float32 integrand, float64 sums);
  * frames: the two bounds of test_device_depth_matrix_matches_oracle (max < 0.5, median < 1e-6);
  * bytes: equal where nothing may move.
CPU side (the law, the table, configuration, header): tests/test_ld_table.py."""
import os
import shutil

import numpy as np
import pytest

import helpers
from oracle import clib
from wayne_amd import _lib, engine, fitsio, lightcurve as lc, run_visit, tools

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI = os.path.join(ROOT, "tests", "fixtures", "mini_visit")
LD = [0.800627, -0.757066, 0.897268, -0.384804]
ATOL = 2e-8


def table_at(wl):
    s = np.clip((np.asarray(wl, dtype=float) - 1.1) / 0.6, 0.0, 1.0)
    return np.stack([0.55 + 0.25 * s, -0.2 - 0.55 * s, 0.5 + 0.4 * s, -0.25 - 0.13 * s], axis=1)


class Case(object):
    """The visit, its engine and the inputs of the three parity cases; references are computed once and kept."""

    def __init__(self):
        v = self.v = helpers.make_visit("small256")
        self.kw = v.frame_kwargs(0)
        self.pg = helpers.product_generator(v, 0)
        self.eng = engine.get_engine(0, v.grism, v.detector, v.calibration, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)
        self.i0, self.i1 = tools.crop_spectrum_ind(v.grism.wl_limits[0], v.grism.wl_limits[1], v.wl)
        K = len(v.sample_mid_points)
        rp0 = np.sqrt(v.depth0.mean())
        z = np.array([1.5, 1.0 + rp0 * 1.0001, 1.0 + rp0 * 0.5, 1.0, 1.0 - rp0 * 0.9999, 0.6, rp0 * 1.0002, rp0 * 0.3, 0.0])
        assert K == z.size
        spec = v.depth0 * (1 + 0.004 * np.sin(np.arange(v.depth0.size) / 300.0))
        z_ecl, hidden = z.copy(), np.zeros(K)
        z_ecl[[0, 5]] = [10.3, 11.0]          # two rows behind the star
        hidden[[0, 5]] = [0.4, 1.0]
        self.table = table_at(v.wl)
        self.inputs = {"spectrum": (z, np.zeros(K), spec),
                       "flat": (z, np.zeros(K), np.full_like(v.depth0, 0.0146)),
                       "eclipse": (z_ecl, hidden, spec)}
        self._got = {}

    def depths(self, name, ld=None):
        z, hidden, spec = self.inputs[name]
        return lc.DeviceDepths(z, hidden, spec, self.table if ld is None else ld)

    def device_matrix(self, dd, slot=0, ctx=None, runs=1):
        ctx = ctx or self.eng.ctx
        ctx.upload(slot, self.pg.build_descriptor(self.eng, **dict(self.kw, planet_signal=dd)))
        for _ in range(runs):
            ctx.run_front(slot)
            got = ctx.debug_depth(slot)
            ctx.run_back(slot)
        return got

    def got(self, name):
        if name not in self._got:
            self._got[name] = self.device_matrix(self.depths(name))
        return self._got[name]


@pytest.fixture(scope="module")
def case(gpu_ctx):
    return Case()


@pytest.mark.parametrize("name", ["spectrum", "flat", "eclipse"])
def test_debug_depth_parity(case, name):
    """Worst |device - numpy law| seen on the MI355X: 4.8e-9 (spectrum), 2.3e-9 (flat), 4.8e-9 (eclipse); against the
    oracle 3.9e-9, 2.3e-9, 3.9e-9."""
    dd = case.depths(name)
    got = case.got(name)
    i0, i1 = case.i0, case.i1
    want = dd.host_matrix()[:, i0:i1]
    assert got.shape == want.shape
    print("k_lightcurve_ld %s: max |device - numpy law| = %.3e" % (name, np.abs(got - want).max()))
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)
    # the oracle, once per wavelength with that wavelength's coefficients
    spec, tab = dd.planet_spectrum[i0:i1], case.table[i0:i1]
    cols = np.arange(0, i1 - i0, 8)
    oracle = np.stack([clib.lc_depths(dd.z_tr, dd.hidden, spec[w:w + 1], tab[w])[:, 0] for w in cols], axis=1)
    print("k_lightcurve_ld %s: max |device - oracle| = %.3e over %d wavelengths" % (
        name, np.abs(got[:, cols] - oracle).max(), cols.size))
    np.testing.assert_allclose(got[:, cols], oracle, rtol=0, atol=ATOL)
    assert got[2].min() > 0 and got[7].min() > 0.01           # rows in transit in every case
    if name == "eclipse":
        np.testing.assert_allclose(got[5], spec / (1 + spec), rtol=0, atol=1e-15)     # fully hidden planet, no transit
    else:
        assert got[0].max() == 0.0 and got[5].min() > 0.01


def test_table_differs_from_single_set(case):
    one = case.device_matrix(case.depths("spectrum", LD))
    assert np.abs(case.got("spectrum") - one).max() > 1e-4


def test_frames_equal_host_matrix(case):
    # replay thrower, noise sources off: the exposure built from the device's matrix equals the one given host_matrix()
    dd = case.depths("eclipse")
    off = dict(add_stellar_noise=False, sky_background=0.0, cosmic_rate=None, add_dark=False, add_read_noise=False)
    a = np.stack([r[0] for r in case.pg.scanning_frame(rng_mode=_lib.RNG_REPLAY, out_dtype=np.float64,
                                                       **dict(case.kw, planet_signal=dd, **off)).reads])
    b = np.stack([r[0] for r in case.pg.scanning_frame(rng_mode=_lib.RNG_REPLAY, out_dtype=np.float64,
                                                       **dict(case.kw, planet_signal=dd.host_matrix(), **off)).reads])
    # ... and differs from the single-set exposure, or the comparison says nothing
    c = np.stack([r[0] for r in case.pg.scanning_frame(rng_mode=_lib.RNG_REPLAY, out_dtype=np.float64,
                                                       **dict(case.kw, planet_signal=case.depths("eclipse", LD), **off)).reads])
    assert np.abs(a - b).max() < 0.5
    assert np.median(np.abs(a - b)) < 1e-6
    assert np.abs(a - c).max() > 0.5


def test_nothing_else_moved(case):
    v = case.v
    fresh = engine.Engine(0, v.grism, v.detector, v.calibration, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)
    try:
        ctx = fresh.ctx
        plain, tabled = case.depths("spectrum", LD), case.depths("spectrum")
        before = case.device_matrix(plain, ctx=ctx)                 # no table was ever set on this context
        with_table = case.device_matrix(tabled, ctx=ctx)
        after = case.device_matrix(plain, ctx=ctx)                  # set -> re-upload without one
        assert before.tobytes() == after.tobytes()
        assert before.tobytes() != with_table.tobytes()
        # ... and set -> cleared on the same upload
        ctx.upload(0, case.pg.build_descriptor(fresh, **dict(case.kw, planet_signal=tabled)))
        ctx.set_limb_darkening(0, None)
        ctx.run_front(0)
        cleared = ctx.debug_depth(0)
        ctx.run_back(0)
        # (the descriptor of a table carries the table's first row as lc_ld: the single-set run of THAT row)
        first_row = case.device_matrix(case.depths("spectrum", list(case.table[0])), ctx=ctx)
        assert cleared.tobytes() == first_row.tobytes()
        # the same bytes in slots 0 and 5 (the two streams), and on a second run
        assert with_table.tobytes() == case.got("spectrum").tobytes()
        assert case.device_matrix(tabled, slot=5, ctx=ctx).tobytes() == with_table.tobytes()
        assert case.device_matrix(tabled, slot=5, ctx=ctx, runs=2).tobytes() == with_table.tobytes()
        ctx.synchronize()
    finally:
        fresh.close()


def test_refusals(case):
    ctx, W = case.eng.ctx, case.i1 - case.i0
    tab = np.ascontiguousarray(case.table[case.i0:case.i1])
    plain = case.depths("spectrum", LD)
    want = case.device_matrix(plain, slot=2)

    def refused(status, table, slot=2):
        with pytest.raises(_lib.WayneError) as e:
            ctx.set_limb_darkening(slot, table)
        assert e.value.status == status

    refused(_lib.E_STATE, tab, slot=201)                       # a slot that is not uploaded
    bad_nan, bad_flux = tab.copy(), tab.copy()
    bad_nan[W // 2, 2] = np.nan
    bad_flux[W - 1] = [5.0, 0.0, 0.0, 0.0]                     # 1 - 5/5 = 0
    for table in (tab[:-1], bad_nan, bad_flux):
        ctx.set_limb_darkening(2, tab)                         # a table is set, then a refused one: the slot runs without any
        refused(_lib.E_INVALID, table)
        ctx.run_front(2)
        got = ctx.debug_depth(2)
        ctx.run_back(2)
        assert got.tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        ctx.set_limb_darkening(2, tab[:, :3])
    # a slot whose depth matrix was uploaded has no device light curve
    ctx.upload(2, case.pg.build_descriptor(case.eng, **dict(case.kw, planet_signal=plain.host_matrix())))
    refused(_lib.E_INVALID, tab)
    ctx.set_limb_darkening(2, None)                            # clearing is never refused
    ctx.run_front(2)
    got = ctx.debug_depth(2)
    ctx.run_back(2)
    np.testing.assert_array_equal(got, plain.host_matrix()[:, case.i0:case.i1])
    ctx.synchronize()


def test_run_visit_with_a_table(case, tmp_path):
    work = str(tmp_path / "visit")
    shutil.copytree(MINI, work)
    nodes = np.linspace(1.05, 1.75, 8)
    with open(os.path.join(work, "params.yml")) as f:
        text = f.read()
    rows = ", ".join("[%s]" % ", ".join(repr(float(x)) for x in row) for row in table_at(nodes))
    text = text.replace("  ldcoeffs:", "  ld_table: {law: claret4, wl_um: [%s], coeffs: [%s]}\n  ldcoeffs:" % (
        ", ".join(repr(float(x)) for x in nodes), rows))
    with open(os.path.join(work, "params.yml"), "w") as f:
        f.write(text)
    obs = run_visit.run(["-p", os.path.join(work, "params.yml"), "--max-exposures", "2"])
    table = lc.LimbDarkening(nodes, table_at(nodes))
    assert obs.ld_table == table
    for n in (1, 2):
        hdr = fitsio.scan(os.path.join(obs.outdir, "%04d_raw.fits" % n))[0][0]
        assert hdr["LDTABLE"] is True and hdr["LDLAW"].strip() == "CLARET4" and hdr["LDNODES"] == 8
        assert hdr["LDHASH"].strip() == table.hash and hdr["LDWLLO"] == 1.05 and hdr["LDWLHI"] == 1.75
        assert hdr["LD1"] == LD[0]
        assert obs.exposure_file_is_whole(n)
    # Observation.generate_lightcurves is the device's matrix: exposure 1 again, by hand
    gen = obs._generate_exposure(obs.exp_start_times[0], 1, prepare_only=True)
    eng, desc, _ = gen._prepared
    gen._prepared = None
    _, mid, _, _ = gen._gen_scanning_sample_times(obs.sample_rate)
    t = obs.exp_start_times[0] + mid / (86400. * 1000.)
    assert obs.device_depths(t).ld_table.shape == (obs.wl.size, 4) and desc._ld_table is not None
    eng.ctx.upload(0, desc)
    eng.ctx.run_front(0)
    got = eng.ctx.debug_depth(0)
    eng.ctx.run_back(0)
    eng.ctx.synchronize()
    i0, i1 = tools.crop_spectrum_ind(obs.grism.wl_limits[0], obs.grism.wl_limits[1], obs.wl)
    want = 1.0 - obs.generate_lightcurves(t)[:, i0:i1]
    print("run_visit: max |device - generate_lightcurves| = %.3e" % np.abs(got - want).max())
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)
    assert want.max() > 1e-3                                   # the fixture's first exposure is in ingress
