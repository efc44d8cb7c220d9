"""GPU: k_lightcurve and k_lightcurve_ld across the (z, rp, spread) plane, against oracle/lc_oracle.c.

Inputs on `small256` with K = 64, as in tests/test_ld_table_gpu.py (upload, run_front, debug_depth, run_back), on every
16th wavelength of the grid: W = 281 bins, more than one pass of the workgroup over the wavelengths and no multiple of
its 256 threads, so that the oracle (63 us per point) can be asked at every column.  One upload carries a whole family of
separations (tests/lightcurve_plane.py `families_of`, from the range of the radius ratios that were uploaded): every
contact at 0.5, 1.01 and 2 guard, 0.01, 0.1 and 0.3 width outside the interval and 2 guard and 0.1 width inside it,
1 + p_hi -+ 2 guard, 0, 1, 1.5, 16 uniform draws, and 0.5 p_lo, 0.6, 2 to fill the 64.

Spectra, each through both kernels: rp = p0 (1 + rel sin(i / 37)) for five (p0, rel), a flat one, a two-valued one (half
of the columns on p_lo, half on p_hi: t = -+1).  The table: the smooth rows of test_ld_table_gpu.table_at with every 7th
column uniform, every 11th (0.9, 0, 0, 0), every 13th (0, 0, 0, 0.9).
Bound: 2e-8 where p_hi <= 0.2 (the project's); for rp 0.3 +- 30 % twice the float32 emulation's worst error of that
family (profiles/lightcurve_plane.json `f32_emulation`, written by tests/test_lightcurve_plane.py) -- the factor of two
for the device's atan2f / sqrtf differing from numpy's float32 by ulps.  The observed worst errors go to the same file
(`device`)."""
import json

import numpy as np
import pytest

import helpers
import lightcurve_plane as lp
from oracle import clib
from wayne_amd import engine, lightcurve as lc, tools

pytestmark = pytest.mark.gpu

K = 64
STEP = 16
ATOL = 2e-8
SPECTRA = {"0.03+-30%": (0.03, 0.3), "0.1208+-2%": (0.1208, 0.02), "0.1208+-15%": (0.1208, 0.15),
           "0.1208+-30%": (0.1208, 0.3), "0.3+-30%": (0.3, 0.3), "flat": (0.1208, 0.0), "two-valued": (0.1208, 0.15)}
SETS = {7: [0.0, 0.0, 0.0, 0.0], 11: [0.9, 0.0, 0.0, 0.0], 13: [0.0, 0.0, 0.0, 0.9]}


def table_at(wl):
    s = np.clip((np.asarray(wl, dtype=float) - 1.1) / 0.6, 0.0, 1.0)
    return np.stack([0.55 + 0.25 * s, -0.2 - 0.55 * s, 0.5 + 0.4 * s, -0.25 - 0.13 * s], axis=1)


class Plane(object):
    def __init__(self):
        v = self.v = helpers.make_visit("small256", K=K)
        assert len(v.sample_mid_points) == K
        wl = v.wl[::STEP].copy()
        self.kw = v.frame_kwargs(0, planet_signal=None, wl=wl, stellar_flux=v.stellar_flux[::STEP].copy())
        self.pg = helpers.product_generator(v, 0)
        self.eng = engine.get_engine(0, v.grism, v.detector, v.calibration, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)
        self.i0, self.i1 = tools.crop_spectrum_ind(v.grism.wl_limits[0], v.grism.wl_limits[1], wl)
        self.N, self.W = wl.size, self.i1 - self.i0
        assert 256 < self.W < 512 and self.W % 256
        # the table: smooth rows, three families of columns (counted from the first uploaded one) overwritten
        self.table = table_at(wl)
        self.owner = np.zeros(self.W, dtype=int)          # 0: the smooth row; 7, 11, 13: the set of SETS
        for every, row in SETS.items():
            cols = np.arange(0, self.W, every)
            self.table[self.i0 + cols] = row
            self.owner[cols] = every
        with open(lp.PROFILE) as f:
            self.f32 = json.load(f)["f32_emulation"]
        self.device = {}

    def spectrum(self, name):
        """The planet spectrum [N] (rp^2) of a case, the family of separations of its uploaded range, and its bound."""
        p0, rel = SPECTRA[name]
        i = np.arange(self.W)
        if name == "two-valued":
            rp = np.where(i % 2 == 0, p0 * (1.0 - rel), p0 * (1.0 + rel))
        else:
            rp = p0 * (1.0 + rel * np.sin(i / 37.0))
        spec = np.full(self.N, p0 * p0)
        spec[self.i0:self.i1] = rp * rp
        p = np.sqrt(spec[self.i0:self.i1])                 # what the descriptor carries
        p_lo, p_hi = float(p.min()), float(p.max())
        fam = lp.families_of(p_lo, p_hi) + [(0.5 * p_lo, "over the centre"), (0.6, "z=0.6"), (2.0, "z=2")]
        assert len(fam) == K
        bound = ATOL if p_hi <= 0.2 else 2.0 * self.f32["%g" % p0]
        return spec, p_lo, p_hi, fam, bound

    def device_matrix(self, dd):
        ctx = self.eng.ctx
        ctx.upload(0, self.pg.build_descriptor(self.eng, **dict(self.kw, planet_signal=dd)))
        ctx.run_front(0)
        got = ctx.debug_depth(0)
        ctx.run_back(0)
        return got

    def oracle(self, z, hidden, spec, table):
        """(columns, depths[K, len(columns)]): a single set at every column; a table at every 4th column and at every
        overwritten one, the oracle called once per coefficient set."""
        s = spec[self.i0:self.i1]
        if table is None:
            return np.arange(self.W), clib.lc_depths(z, hidden, s, lp.LD)
        cols = np.flatnonzero((np.arange(self.W) % 4 == 0) | (self.owner > 0))
        want = np.empty((z.size, cols.size))
        for every, row in SETS.items():
            sel = self.owner[cols] == every
            want[:, sel] = clib.lc_depths(z, hidden, s[cols[sel]], row)
        for j in np.flatnonzero(self.owner[cols] == 0):
            w = cols[j]
            want[:, j] = clib.lc_depths(z, hidden, s[w:w + 1], table[self.i0 + w])[:, 0]
        return cols, want


@pytest.fixture(scope="module")
def plane(gpu_ctx):
    p = Plane()
    yield p
    if p.device:
        lp.record("device", p.device)


@pytest.mark.parametrize("kernel", ["k_lightcurve", "k_lightcurve_ld"])
@pytest.mark.parametrize("name", list(SPECTRA))
def test_plane_against_the_oracle(plane, name, kernel):
    """Worst |device - oracle| seen on the MI355X, single set / table (profiles/lightcurve_plane.json, `device`):
    rp 0.03 +-30 % 1.2e-9 / 1.6e-9; 0.1208 +-2 % 4.2e-9 / 6.0e-9, +-15 % 5.4e-9 / 7.2e-9, +-30 % 7.5e-9 / 8.1e-9; flat
    2.4e-9 / 3.2e-9; two-valued 4.8e-9 / 8.3e-9 (bound 2e-8); rp 0.3 +-30 % 4.0e-8 / 4.6e-8 (bound 7.0e-8).  With the band
    blind to the width the rows next to a contact of the 0.3 +-30 % spectrum were off by a further 1.3e-7."""
    spec, p_lo, p_hi, fam, bound = plane.spectrum(name)
    z = np.array([v for v, _ in fam])
    labels = [lab for _, lab in fam]
    hidden = np.zeros(K)
    table = plane.table if kernel == "k_lightcurve_ld" else None
    got = plane.device_matrix(lc.DeviceDepths(z, hidden, spec, lp.LD if table is None else table))
    assert got.shape == (K, plane.W) and np.isfinite(got).all()
    cols, want = plane.oracle(z, hidden, spec, table)
    err = np.abs(got[:, cols] - want)
    routes = [lp.route(v, p_lo, p_hi) for v in z]
    by_route = {r: float(err[[i for i in range(K) if routes[i] == r]].max()) for r in sorted(set(routes))}
    print("%s %s: [p_lo, p_hi] = [%.6f, %.6f], %d columns compared, bound %.2e, worst |device - oracle| = %.3e  (%s)" % (
        kernel, name, p_lo, p_hi, cols.size, bound, err.max(),
        ", ".join("%s %.2e" % kv for kv in by_route.items())))
    plane.device.setdefault(name, {"bound": bound})[kernel] = float("%.3g" % err.max())
    # every route this spectrum has was taken, and every case is compared
    assert set(routes) == ({"none", "direct", "flat"} if name == "flat" else {"none", "direct", "cheb"})
    worst_row = err.max(axis=1)
    bad = [(labels[i], routes[i], float(worst_row[i])) for i in range(K) if not worst_row[i] <= bound]
    assert not bad, bad
    # the band's edge and the interval's end are straddled at every contact, both sides within the bound (above)
    r = dict(zip(labels, routes))
    for c, _, _ in lp.contacts(p_lo, p_hi):
        assert r["%s outside 0.5 guard" % c] == "direct" != r["%s outside 1.01 guard" % c]
        # (a flat spectrum's interval has no inside: 2 guard beyond one end is 2 guard beyond the other)
        assert r["%s outside 2 guard" % c] != "direct" and (name == "flat" or r["%s inside 2 guard" % c] == "direct")
    # without a transit: exactly 0
    out = z >= 1.0 + p_hi
    assert out.sum() >= 3 and not got[out].any()
    assert all(routes[i] == "none" for i in np.flatnonzero(out))
    assert got[labels.index("z=0")].min() > 0.9 * p_lo * p_lo


HIDDEN_MODES = ("none", "zeros", "behind")


def negative_case(plane, name, kernel, mode, planted):
    spec, p_lo, p_hi, fam, _ = plane.spectrum(name)
    z = np.array([v for v, _ in fam])
    hidden = None
    if mode != "none":
        hidden = np.zeros(K)
    if mode == "behind":
        z[[K - 3, K - 2]] = [10.3, 11.0]                   # two rows behind the star
        hidden[[K - 3, K - 2]] = [0.4, 1.0]
    spec = spec.copy()
    spec[[plane.i0 + w for w in planted]] = -1e-4
    with np.errstate(invalid="ignore"):
        p = np.sqrt(spec[plane.i0:plane.i1])
    assert np.nanmin(p) == p_lo and np.nanmax(p) == p_hi   # the planted columns are not the ends of the range
    table = plane.table if kernel == "k_lightcurve_ld" else None
    return plane.device_matrix(lc.DeviceDepths(z, hidden, spec, lp.LD if table is None else table))


@pytest.mark.parametrize("kernel", ["k_lightcurve", "k_lightcurve_ld"])
@pytest.mark.parametrize("name", ["0.1208+-2%", "flat"])
def test_negative_spectrum_elements(plane, name, kernel):
    """A negative element of the spectrum reaches the device as a NaN radius ratio: its column is exactly 0 -- a planet
    of no size blocks and emits nothing -- and every other column is what it is without it: in the first uploaded
    wavelength (where the scan for [p_lo, p_hi] starts), in the middle, in both; without a hidden vector, with zeros,
    with two rows behind the star.  Before the fixes, seen on the MI355X without a hidden vector: planted in the first
    wavelength the whole matrix was 0 (p_lo = p_hi = NaN from the upload's scan), and the flat path of k_lightcurve left
    its one sample, 1.62e-2, in a column planted in the middle; with a hidden vector the eclipse term p^2 hidden / (1 + p^2)
    is NaN whatever `hidden` holds (read from the code: not run, the NaN depths would have gone on into the thrower)."""
    W = plane.W
    plantings = ([0], [W // 2], [0, W // 2]) if name != "flat" else ([0], [W // 2])
    for mode in HIDDEN_MODES:
        clean = negative_case(plane, name, kernel, mode, [])
        assert np.isfinite(clean).all() and clean.max() > 0.01
        if mode == "behind":
            assert clean[K - 2].min() > 0.01               # the fully hidden planet's row: f / (1 + f)
        for planted in plantings:
            got = negative_case(plane, name, kernel, mode, planted)
            assert np.isfinite(got).all(), (mode, planted)
            assert not got[:, planted].any(), (mode, planted)
            keep = np.setdiff1d(np.arange(W), planted)
            assert got[:, keep].tobytes() == clean[:, keep].tobytes(), (mode, planted)


def test_no_finite_radius_ratio(plane):
    # every element negative: no column is in transit, with or without a hidden vector
    spec, p_lo, p_hi, fam, _ = plane.spectrum("0.1208+-2%")
    z = np.array([v for v, _ in fam])
    for hidden in (None, np.full(K, 0.5)):
        for ld in (lp.LD, plane.table):
            got = plane.device_matrix(lc.DeviceDepths(z, hidden, np.full(plane.N, -0.01), ld))
            assert got.shape == (K, plane.W) and not got.any()
