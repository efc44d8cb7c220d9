"""Device-side spectral extraction: the plan handed to the device, and the caller's side of what comes back.

An exposure's reads are 67 MB (float32, full array); what a light-curve consumer keeps of them is one column spectrum
per read interval, ~120 KB.  With an `Extraction` set on a slot (Context.set_extraction, or `extraction=` on
scanning_frame / staring_frame / VisitRunner / Observation.frame_options) the device forms, behind the ramp kernel,

    spectra[j, x]   j = 0 .. R-1: the electrons of read interval j in column x, summed over the interval's row window,
                    linearised, dark-subtracted, gain-corrected and sky-subtracted; j = R: the same from the last read
                    alone over the whole scan's rows
    sky[j]          the fitted sky level of product j (electrons per second per unit of the master-sky template)

(the law: include/wayne_hip.h, wayne_extract_desc) and only those cross PCIe.  Star-fixed column channels can still be
formed here: `channel_weights(...) @ spectra[:R].sum(0)` (up the ramp) or `... @ spectra[R]` (last read).

Wavelength-binned channels are opt-in (`channels=` of Extraction / ExtractionOptions / the frames, CLI --channels
LO:HI:N): the grism's dispersion depends on the star's height, and during a scan every detector row is lit while the star
sits at another height, so lines of constant wavelength are slanted against the columns -- one column-to-wavelength
solution for all rows errs by up to 104 A (2.3 px) over +-200 px on G141, a linear solution per row (`row_solution`) by
0.41 A (G102: 60 A and 0.28 A).  With `Channels(edges_um)` and that per-row solution lambda_y(u) = wl_a[y] + wl_b[y] u the device bins every
window pixel into the channels by fractional column coverage, dividing it first (flat=True, the default) by the flat
cube evaluated at the pixel's wavelength -- the factor the simulator multiplied in -- and hands back
`channels` [R + 1, C] with the spectra (the law: include/wayne_hip.h, wayne_channels_desc).  The sky level is the column
extraction's.  Not covered: resampling in y, other grism orders, the direct image, merging per-rank
.npz files, a flat-fielded sky fit.  Fitting stays with the caller.

Variances are opt-in (`variance=` of Extraction / ExtractionOptions / the frames, CLI --variances [RN]): every pixel
of a window carries var = max(v, 0) + rn^2 q^2 -- Poisson on its own electrons v (the term the extraction sums, cleaned
under rejection) plus the read noise rn of a difference of two reads (20 e- by default, as CosmicRejection.read_noise)
through its own gain factor q = 1 / pfl -- and the device, which alone sees the pixels, sums it beside the flux, in the
same order and from the same loads: `spectra_var` [R + 1, S], `sky_var` [R + 1] and, with channels, `channels_var`
[R + 1, C] come back with the spectra (the law: include/wayne_hip.h, wayne_variance_desc).  The sky level's variance
enters a column as B^2 sky_var and a channel as Q^2 sky_var.  Left out: the covariance between a background column's
own flux and the sky level; the correlation between neighbouring channels that share a pixel (and the sky level); the
correlation of read intervals through the read they share -- in a sum over consecutive intervals the Poisson parts add
but the read noise is that of the first and the last read alone, so the variance of `channels[:R].sum(0)` is
`channels_var[:R].sum(0)` with its read-noise part replaced by the last-read product's (with a second extraction at
read_noise = 0: cv0[:R].sum(0) + cv[R] - cv0[R]); the variance of a rejected pixel's replacement, taken from the
replacement's own value.

Optimal (profile-weighted) extraction is opt-in on top of the variances (`optimal=` of Extraction / ExtractionOptions /
the frames, CLI --optimal [H]): the box extraction sums every row of a window, the margin rows that hold only read noise
and sky included; `optimal` [R + 1, S] weighs a pixel by the share P of the column's light the window's own profile over
2H + 1 columns (H = 8 by default, 1 .. 16) gives it, against the variance V of that model: sum(P d / V) / sum(P P / V),
with `optimal_var` [R + 1, S] = 1 / sum(P P / V) plus the sky level's share (the law: include/wayne_hip.h,
wayne_optimal_desc).  A column without a 3-sigma source over its 2H + 1 columns keeps the box values to the bit.  V is a
model variance (a data variance biased the flux by -0.09 %) and P is clamped at 0 but not renormalised (renormalising
turned the margin rows' noise into flux: +0.16 %, +9.5 % on a nearly unlit interval).  Limits: the profile's own noise is
not in optimal_var, which is too small on a nearly unlit interval (an ensemble showed 1.64 times it); the intervals'
correlation through shared reads is as for spectra_var.  Not covered: a profile from a PSF model or a polynomial fit along the
dispersion, iterating the profile, rejecting on the optimal residuals, the direct image.

A profile formed once per visit: `Optimal(profile=..., deliver_profile=...)`.  The exposure's own profile carries its own
noise, common to the 2H + 1 columns it is formed from, so it adds coherently over the columns of a channel.  With
`deliver_profile` the planes S1 of every window pixel come back too (Exposure.profile_planes; fetched by a call of its
own); ProfileSum adds those of several exposures and normalises them, and `profile=` (a Profile, or the {profile_key:
Profile} of VisitRunner.build_profile) makes the weights come from that sum (the law: include/wayne_hip.h).  Limits: the
profile is fixed on the detector (sub-pixel drift, forward against reverse scans), a nearly unlit interval has a profile
of noise.

Cosmic-ray rejection is opt-in (`crrej=` of Extraction / ExtractionOptions / the frames, CLI --reject-cosmics): on each
read interval's difference image I a pixel at least 7 px inside the frame and in the plan's rows is flagged when it
exceeds the largest of its eight plus-shaped stencil neighbours (y+-1, y+-2, x+-1, x+-2), m8, by d > 0 with
d^2 > k^2 (rn^2 + max(m8, 0)); a flagged pixel counts as the mean of the middle two of its four row neighbours (along the
dispersion, never along the scan), in its interval's product and in the last-read product.  Defaults k = 8 and
rn = 20 e- (sqrt(2) x 14.1 e-, the read noise of a difference of two reads).  On CPU-oracle reads the law flagged 73 of 73
hits of a cfg3 exposure with no false flag at k = 6 and 8 (1 false at k = 5, 6 at k = 4) and 16 of 16 on small256 /
stare256 at k = 4 .. 8, leaving 0.07-0.12 % of the hits' electrons.  `rejected` [R + 1] comes back with the spectra: the
flags in each product's window ((pixel, interval) pairs for the last-read product).  Not covered: hits on adjacent
pixels of one interval (they shield each other), the 7-pixel frame margin, optimal extraction, the direct image.
"""
import hashlib

import numpy as np

from . import _lib, tools
from . import grism as grism_mod

LINEARISE, DARK, GAIN, SKY, LAST_READ = _lib.X_LINEARISE, _lib.X_DARK, _lib.X_GAIN, _lib.X_SKY, _lib.X_LAST_READ
ALL = _lib.X_ALL
ROW_MARGIN = 14
BG_COLS = (6, 26)           # bordered columns left of the first-order spectrum


class CosmicRejection(object):
    """Cosmic-ray rejection of an extraction (wayne_crrej_desc): the threshold `k` in sigma (finite, > 0) and the read
    noise `read_noise` of a difference image in electrons (finite, >= 0)."""

    def __init__(self, k=8.0, read_noise=20.0):
        k, read_noise = float(k), float(read_noise)
        if not (np.isfinite(k) and k > 0.0):
            raise ValueError("CosmicRejection: k must be finite and > 0")
        if not (np.isfinite(read_noise) and read_noise >= 0.0):
            raise ValueError("CosmicRejection: read_noise must be finite and >= 0")
        self.k, self.read_noise = k, read_noise

    @staticmethod
    def coerce(crrej):
        """`crrej=` -> a CosmicRejection or None: None and False are off, True the defaults."""
        if crrej is None or crrej is False:
            return None
        if crrej is True:
            return CosmicRejection()
        if not isinstance(crrej, CosmicRejection):
            raise TypeError("crrej: None, True or an extraction.CosmicRejection")
        return crrej

    def desc(self):
        d = _lib.CrrejDesc()
        d.k, d.read_noise_e = self.k, self.read_noise
        return d


class Variances(object):
    """Variances of an extraction's spectra, sky levels and channels (wayne_variance_desc): `read_noise`, the noise of a
    difference of two reads in electrons (finite, >= 0; the meaning and default of CosmicRejection.read_noise)."""

    def __init__(self, read_noise=20.0):
        read_noise = float(read_noise)
        if not (np.isfinite(read_noise) and read_noise >= 0.0):
            raise ValueError("Variances: read_noise must be finite and >= 0")
        self.read_noise = read_noise

    @staticmethod
    def coerce(variance):
        """`variance=` -> a Variances or None: None and False are off, True the defaults."""
        if variance is None or variance is False:
            return None
        if variance is True:
            return Variances()
        if not isinstance(variance, Variances):
            raise TypeError("variance: None, True or an extraction.Variances")
        return variance

    def desc(self):
        d = _lib.VarianceDesc()
        d.read_noise = self.read_noise
        return d


class Profile(object):
    """A profile for the optimal extraction of a visit's exposures (wayne_exposure_set_optimal_profile): `planes`
    [sum_p rows_p, S] float64 -- the windows of the R + 1 products one behind the other, rows relative to the window -- and
    `rows` [R + 1], the window heights they were made for.  An exposure whose windows have other heights is refused when it
    is run.  `exposures`: how many exposures' planes were added up (0: not known)."""

    def __init__(self, planes, rows, exposures=0):
        rows = tuple(int(r) for r in rows)
        planes = np.array(planes, dtype=np.float64, order="C")      # (a copy of its own, read-only: `tag` names its content)
        if not 2 <= len(rows) <= _lib.EXTRACT_PRODUCTS or min(rows[:-1]) < 1 or rows[-1] < 0:
            raise ValueError("Profile: rows holds the heights of the R read intervals' windows and of the last read's")
        if planes.ndim != 2 or planes.shape[0] != sum(rows):
            raise ValueError("Profile: planes must be [sum(rows), S]")
        if not np.isfinite(planes).all():
            raise ValueError("Profile: planes must be finite")
        planes.setflags(write=False)
        self.planes, self.rows, self.exposures = planes, rows, int(exposures)
        # 64 bits of a cryptographic hash of heights and content, formed once: what a slot that already holds this
        # profile recognises it by (wayne_exposure_set_optimal_profile_tagged), at no cost per exposure
        h = hashlib.blake2b(np.asarray(rows, dtype=np.int64).tobytes(), digest_size=8)
        h.update(planes)
        self.tag = int.from_bytes(h.digest(), "little") or 1

    def window(self, p):
        """The profile of product p's window: a view [rows_p, S]."""
        at = sum(self.rows[:p])
        return self.planes[at:at + self.rows[p]]


def window_heights(plan):
    """The heights of a plan's R + 1 windows, as the profile planes lay them out (the last read's window counts whether
    the plan forms that product or not: its rows are zeros then)."""
    return tuple(int(hi) - int(lo) for lo, hi in plan.row_windows)


def profile_key(plan, scan_speed):
    """What exposures must share to share a profile: (the plan's window heights, the scan's direction +1 / -1 / 0)."""
    speed = float(getattr(scan_speed, "value", scan_speed) or 0.0)
    return window_heights(plan), int(np.sign(speed))


class ProfileSum(object):
    """Adds the delivered planes (S1) of several exposures with equal window heights and normalises the sum: a
    flux-weighted mean profile, with no division by a noisy S0."""

    def __init__(self):
        self.rows, self.total, self.n = None, None, 0

    def add(self, plan, planes):
        rows = window_heights(plan)
        planes = np.asarray(planes, dtype=np.float64)
        if planes.ndim != 2 or planes.shape[0] != sum(rows):
            raise ValueError("ProfileSum: planes must be [sum of the plan's window heights, S]")
        if self.rows is None:
            self.rows, self.total = rows, np.zeros_like(planes)
        elif rows != self.rows or planes.shape != self.total.shape:
            raise ValueError("ProfileSum: the exposure's window heights %s differ from %s" % (rows, self.rows))
        self.total = self.total + planes
        self.n += 1
        return self

    def profile(self):
        """The Profile: every column of every window divided by its sum over the window's rows; a column whose sum is
        not positive gets zeros (W = 0 there: the box values)."""
        if self.rows is None:
            raise ValueError("ProfileSum: nothing was added")
        out = np.zeros_like(self.total)
        at = 0
        for r in self.rows:
            w = self.total[at:at + r]
            tot = w.sum(axis=0)
            good = tot > 0.0
            out[at:at + r][:, good] = w[:, good] / tot[good]
            at += r
        return Profile(out, self.rows, self.n)


class Optimal(object):
    """Optimal (profile-weighted) extraction beside the box extraction (wayne_optimal_desc): `half_width`, the columns on
    either side of a column whose light forms its profile (an integer in 1 .. 16).  It needs the variances.  `profile` (a
    Profile): the weights come from it and not from the exposure's own light (half_width then enters through the
    detection test alone); as {profile_key: Profile} (VisitRunner.build_profile) an ExtractionOptions picks each
    exposure's by its window heights and scan direction.  `deliver_profile`: the exposure's own planes S1 come back too (Exposure.profile_planes; the raw
    material of a ProfileSum).  `channels` (the plan must carry channels): the pixels' weighted terms are binned into the
    plan's wavelength channels too -- channels_opt and channels_opt_var [R + 1, C] (wayne_exposure_set_optimal_channels);
    meant for a supplied profile: with the exposure's own, channels_opt_var is too small (README)."""

    def __init__(self, half_width=8, profile=None, deliver_profile=False, channels=False):
        if isinstance(half_width, bool) or int(half_width) != half_width:
            raise ValueError("Optimal: half_width must be an integer")
        half_width = int(half_width)
        if not 1 <= half_width <= _lib.MAX_OPTIMAL_HALF_WIDTH:
            raise ValueError("Optimal: half_width must lie in 1 .. %d" % _lib.MAX_OPTIMAL_HALF_WIDTH)
        if isinstance(profile, dict):
            if not all(isinstance(v, Profile) for v in profile.values()):
                raise TypeError("Optimal: profile is None, an extraction.Profile or {profile_key: Profile}")
        elif profile is not None and not isinstance(profile, Profile):
            raise TypeError("Optimal: profile is None, an extraction.Profile or {profile_key: Profile}")
        self.half_width = half_width
        self.profile = profile
        self.deliver_profile = bool(deliver_profile)
        self.channels = bool(channels)

    def with_profile(self, profile, deliver_profile=False, channels=None):
        """The same options with another `profile` and `deliver_profile` (and, if given, `channels`)."""
        return Optimal(self.half_width, profile, deliver_profile, self.channels if channels is None else channels)

    @staticmethod
    def coerce(optimal):
        """`optimal=` -> an Optimal or None: None and False are off, True the defaults."""
        if optimal is None or optimal is False:
            return None
        if optimal is True:
            return Optimal()
        if not isinstance(optimal, Optimal):
            raise TypeError("optimal: None, True or an extraction.Optimal")
        return optimal

    def desc(self):
        d = _lib.OptimalDesc()
        d.half_width = self.half_width
        return d


MAX_CHANNELS = _lib.MAX_CHANNELS
MAX_HULL = _lib.MAX_CHANNEL_HULL      # widest column hull of a channel plan (kChanMaxHull)


class Channels(object):
    """Wavelength channels of an extraction (wayne_channels_desc): `edges_um` [C + 1], finite and increasing, 1 <= C <=
    256; `flat`: divide every pixel by the flat cube at its wavelength (WAYNE_C_FLAT)."""

    def __init__(self, edges_um, flat=True):
        e = np.array(edges_um, dtype=np.float64)
        if e.ndim != 1 or not 2 <= e.size <= MAX_CHANNELS + 1:
            raise ValueError("Channels: between 1 and %d channels (edges_um holds one more)" % MAX_CHANNELS)
        if not np.isfinite(e).all():
            raise ValueError("Channels: edges_um must be finite")
        if not (np.diff(e) > 0.0).all():
            raise ValueError("Channels: edges_um must increase")
        self.edges_um, self.flat = e, bool(flat)

    @staticmethod
    def linear(lo_um, hi_um, n):
        """`n` channels of equal width between lo_um and hi_um."""
        n = int(n)
        if n < 1:
            raise ValueError("Channels: between 1 and %d channels" % MAX_CHANNELS)
        return Channels(np.linspace(float(lo_um), float(hi_um), n + 1))

    @staticmethod
    def coerce(channels):
        """`channels=` -> a Channels or None: None and False are off."""
        if channels is None or channels is False:
            return None
        if not isinstance(channels, Channels):
            raise TypeError("channels: None or an extraction.Channels")
        return channels

    def with_flat(self, flat):
        return Channels(self.edges_um, flat)

    @property
    def n(self):
        return self.edges_um.size - 1


def channel_hull(channels, row_solution, row_windows, steps=ALL):
    """The bordered columns [u_lo, u_hi) the channels can touch on the rows of the windows that are formed (as
    plan::channels_desc_error computes them): min_y floor(ua_0(y)) to max_y ceil(ua_C(y)), clamped to [0, S].  Raises
    ValueError for what wayne_exposure_set_channels refuses."""
    wl_a, wl_b = (np.asarray(v, dtype=np.float64) for v in row_solution)
    if wl_a.ndim != 1 or wl_a.shape != wl_b.shape:
        raise ValueError("row_solution: (wl_a [S], wl_b [S])")
    S = wl_a.size
    w = np.asarray(row_windows)
    w = w if steps & LAST_READ else w[:-1]
    rows = np.zeros(S, dtype=bool)
    for lo, hi in w:
        rows[int(lo):int(hi)] = True
    a, b = wl_a[rows], wl_b[rows]
    if not np.isfinite(a).all():
        raise ValueError("row_solution: wl_a must be finite on every row of a window")
    if not (np.isfinite(b) & (b > 0.0)).all():
        raise ValueError("row_solution: wl_b must be finite and > 0 on every row of a window")
    with np.errstate(over="ignore", invalid="ignore"):
        ua0, uaC = (channels.edges_um[0] - a) / b, (channels.edges_um[-1] - a) / b
    if not (np.isfinite(ua0).all() and np.isfinite(uaC).all()):
        raise ValueError("row_solution: a channel edge has no finite column on a row of a window")
    lo = min(float(S), float(np.floor(ua0).min())) if a.size else float(S)
    hi = max(0.0, float(np.ceil(uaC).max())) if a.size else 0.0
    lo = min(max(lo, 0.0), float(S))
    hi = min(max(hi, lo), float(S))
    if hi - lo > MAX_HULL:
        raise ValueError("channels: the column hull is wider than %d columns" % MAX_HULL)
    return int(lo), int(hi)


class Extraction(object):
    """The plan of one exposure's extraction: `row_windows` [(lo, hi)] * (R + 1) -- bordered rows, half open, read
    interval j at index j and the last-read product at index R -- the background columns and the step mask (LINEARISE |
    DARK | GAIN | SKY | LAST_READ; a step that is off: see the WAYNE_X_* bits).  `crrej` (None, True or a
    CosmicRejection): cosmic rays are rejected on the difference images first; it needs the GAIN step.  `channels` (None
    or a Channels) with `row_solution` = (wl_a [S], wl_b [S]): the window pixels are also binned into wavelength
    channels, row y by lambda_y(u) = wl_a[y] + wl_b[y] u at bordered column coordinate u.  `variance` (None, True or a
    Variances): variances come back with the spectra, the sky levels and the channels; it needs the GAIN step.  `optimal`
    (None, True or an Optimal): the profile-weighted spectra and their variances come back too; it needs `variance`."""

    def __init__(self, row_windows, bg_cols=BG_COLS, steps=ALL, crrej=None, channels=None, row_solution=None,
                 variance=None, optimal=None):
        w = np.asarray(row_windows, dtype=np.int64)
        if w.ndim != 2 or w.shape[1] != 2 or not 2 <= w.shape[0] <= _lib.EXTRACT_PRODUCTS:
            raise ValueError("row_windows: (lo, hi) for each of the R read intervals and for the last read")
        self.row_windows = w
        self.bg_cols = (int(bg_cols[0]), int(bg_cols[1]))
        self.steps = int(steps)
        self.crrej = CosmicRejection.coerce(crrej)
        self.channels = Channels.coerce(channels)
        self.variance = Variances.coerce(variance)
        if self.variance is not None and not self.steps & GAIN:
            raise ValueError("variance needs the GAIN step: a variance is in electrons^2")
        self.optimal = Optimal.coerce(optimal)
        if self.optimal is not None and self.variance is None:
            raise ValueError("optimal needs variance: the weights are formed from the variances")
        if self.optimal is not None and self.optimal.channels and self.channels is None:
            raise ValueError("optimal channels need channels: they are binned by the channels' edges and row solution")
        self.row_solution = None
        self.hull = None              # (u_lo, u_hi): the bordered columns the channels can touch
        if self.channels is not None:
            if row_solution is None:
                raise ValueError("channels need a row_solution (wl_a, wl_b)")
            self.row_solution = tuple(np.array(v, dtype=np.float64) for v in row_solution)
            self.hull = channel_hull(self.channels, self.row_solution, w, self.steps)

    def with_crrej(self, crrej):
        """The same plan with another `crrej`."""
        return Extraction(self.row_windows, self.bg_cols, self.steps, crrej, self.channels, self.row_solution,
                          self.variance, self.optimal)

    def with_channels(self, channels, row_solution=None):
        """The same plan with other `channels` (None: without); `row_solution` defaults to the plan's own."""
        return Extraction(self.row_windows, self.bg_cols, self.steps, self.crrej, channels,
                          self.row_solution if row_solution is None else row_solution, self.variance, self.optimal)

    def with_variance(self, variance):
        """The same plan with another `variance` (without one, also without `optimal`, which needs it)."""
        return Extraction(self.row_windows, self.bg_cols, self.steps, self.crrej, self.channels, self.row_solution,
                          variance, self.optimal if Variances.coerce(variance) is not None else None)

    def with_optimal(self, optimal):
        """The same plan with another `optimal`."""
        return Extraction(self.row_windows, self.bg_cols, self.steps, self.crrej, self.channels, self.row_solution,
                          self.variance, optimal)

    @property
    def mask_rows(self):
        """(lo, hi): the rows the rejection's flag plane covers -- the union's hull of the windows that are formed."""
        w = self.row_windows if self.steps & LAST_READ else self.row_windows[:-1]
        return int(w[:, 0].min()), int(w[:, 1].max())

    @property
    def row_lo(self):
        return self.row_windows[:, 0].copy()

    @property
    def row_hi(self):
        return self.row_windows[:, 1].copy()

    def desc(self):
        d = _lib.ExtractDesc()
        d.steps = self.steps & 0xFFFFFFFF
        n = self.row_windows.shape[0]
        d.row_lo[:n] = [int(v) for v in self.row_windows[:, 0]]
        d.row_hi[:n] = [int(v) for v in self.row_windows[:, 1]]
        d.bg_col_lo, d.bg_col_hi = self.bg_cols
        return d


OWN = object()             # `channels=` of ExtractionOptions.plan: the options' own


class ExtractionOptions(object):
    """Extraction planned per exposure: what `extraction=` takes where the star moves from exposure to exposure
    (Observation.frame_options, VisitRunner).  ExposureGenerator turns it into that exposure's Extraction (plan)."""

    def __init__(self, margin=ROW_MARGIN, bg_cols=BG_COLS, steps=ALL, crrej=None, channels=None, variance=None,
                 optimal=None):
        self.margin, self.bg_cols, self.steps = int(margin), (int(bg_cols[0]), int(bg_cols[1])), int(steps)
        self.crrej = CosmicRejection.coerce(crrej)
        self.channels = Channels.coerce(channels)
        self.variance = Variances.coerce(variance)
        self.optimal = Optimal.coerce(optimal)
        if self.optimal is not None and self.variance is None:
            raise ValueError("optimal needs variance: the weights are formed from the variances")

    def with_optimal(self, optimal):
        """The same options with another `optimal`."""
        return ExtractionOptions(self.margin, self.bg_cols, self.steps, self.crrej, self.channels, self.variance, optimal)

    def plan(self, grism, wl, x_ref, y_ref, scan_speed, read_times, sub_scale, S, channels=OWN):
        """This exposure's Extraction; `channels` (a Channels or None) replaces the options' own."""
        channels = self.channels if channels is OWN else Channels.coerce(channels)
        sol = None if channels is None else row_solution(grism, x_ref, y_ref, sub_scale, S)
        plan = Extraction(row_windows(grism, wl, x_ref, y_ref, scan_speed, read_times, sub_scale, S, self.margin),
                          self.bg_cols, self.steps, self.crrej, channels, sol, self.variance, self.optimal)
        return pick_profile(plan, scan_speed)


def pick_profile(plan, scan_speed):
    """`plan` with its exposure's own Profile where its Optimal carries {profile_key: Profile} (otherwise as it is)."""
    if plan is None or plan.optimal is None or not isinstance(plan.optimal.profile, dict):
        return plan
    key = profile_key(plan, scan_speed)
    if key not in plan.optimal.profile:
        raise ValueError("optimal: no profile for window heights %s and scan direction %+d" % key)
    return plan.with_optimal(plan.optimal.with_profile(plan.optimal.profile[key], plan.optimal.deliver_profile))


def for_exposure(extraction, grism, wl, x_ref, y_ref, scan_speed, read_times, sub_scale, S, crrej=None, channels=None,
                 variance=None, optimal=None):
    """`extraction=` of a frame -> that exposure's Extraction: None stays None, an Extraction is taken as it is, True is
    the default plan and an ExtractionOptions its own.  `crrej=` of the frame, when given, replaces the plan's; so does
    `channels=` (a Channels), with the row solution planned for this exposure, and so does `variance=` (True or a
    Variances) and `optimal=` (True or an Optimal; without variances on the plan it is an error)."""
    if optimal is not None:
        plan = for_exposure(extraction, grism, wl, x_ref, y_ref, scan_speed, read_times, sub_scale, S, crrej, channels,
                            variance)
        if plan is None:
            if optimal is not False:
                raise ValueError("optimal needs an extraction")
            return None
        return pick_profile(plan.with_optimal(optimal), scan_speed)
    if variance is not None:
        if extraction is None or extraction is False:
            if variance is not False:
                raise ValueError("variance needs an extraction")
            return for_exposure(extraction, grism, wl, x_ref, y_ref, scan_speed, read_times, sub_scale, S, crrej, channels)
        return for_exposure(extraction, grism, wl, x_ref, y_ref, scan_speed, read_times, sub_scale, S, crrej,
                            channels).with_variance(variance)
    if extraction is None or extraction is False:
        if crrej is not None and crrej is not False:
            raise ValueError("crrej needs an extraction")
        if channels is not None and channels is not False:
            raise ValueError("channels need an extraction")
        return None
    if channels is not None:
        # the replaced channels are never planned: only the ones asked for here are, by the one planner
        channels = Channels.coerce(channels)
        if isinstance(extraction, Extraction):
            plan = extraction.with_channels(channels, None if channels is None else row_solution(grism, x_ref, y_ref, sub_scale, S))
        else:
            if extraction is True:
                extraction = ExtractionOptions()
            if not isinstance(extraction, ExtractionOptions):
                raise TypeError("extraction: None, True, an extraction.Extraction or an extraction.ExtractionOptions")
            plan = extraction.plan(grism, wl, x_ref, y_ref, scan_speed, read_times, sub_scale, S, channels=channels)
        return plan if crrej is None else plan.with_crrej(crrej)
    if crrej is not None:
        plan = for_exposure(extraction, grism, wl, x_ref, y_ref, scan_speed, read_times, sub_scale, S)
        return plan.with_crrej(crrej)
    if isinstance(extraction, Extraction):
        return extraction
    if extraction is True:
        extraction = ExtractionOptions()
    if not isinstance(extraction, ExtractionOptions):
        raise TypeError("extraction: None, True, an extraction.Extraction or an extraction.ExtractionOptions")
    return extraction.plan(grism, wl, x_ref, y_ref, scan_speed, read_times, sub_scale, S)


def row_windows(grism, wl, x_ref, y_ref, scan_speed, read_times, sub_scale, S, margin=ROW_MARGIN):
    """The default plan: for each read interval (t0, t1) the bordered rows the first-order spectrum crosses in it, from
    floor(y* + dy_min + v t0) - margin to ceil(y* + dy_max + v t1) + margin + 1, clamped to [5, S - 5]; y* = y_ref -
    sub_scale + 5 and dy_min / dy_max the extremes of the trace's y offset from the star over the wavelength grid cropped
    to the grism's limits.  The last-read window is that of (0, t_R).  scan_speed in px / s (0: a staring exposure, the
    same window for every product); read_times in s.  -> int array [R + 1, 2]."""
    wl = np.asarray(wl, dtype=float)
    i0, i1 = tools.crop_spectrum_ind(grism.wl_limits[0], grism.wl_limits[1], wl)
    tr = grism.get_trace(x_ref + 0.5, y_ref + 0.5)
    dy = np.asarray(tr.wl_to_y(wl[i0:i1]), dtype=float) - (y_ref + 0.5)
    v = float(scan_speed or 0.0)
    y0 = y_ref - sub_scale + 5.0 + dy.min()
    y1 = y_ref - sub_scale + 5.0 + dy.max()
    read_times = np.asarray(read_times, dtype=float)
    spans = list(zip(np.concatenate([[0.0], read_times[:-1]]), read_times)) + [(0.0, read_times[-1])]
    out = np.empty((len(spans), 2), dtype=np.int64)
    for j, (t0, t1) in enumerate(spans):
        lo = int(np.floor(y0 + v * t0)) - margin
        hi = int(np.ceil(y1 + v * t1)) + margin + 1
        out[j] = max(lo, 5), min(hi, S - 5)
    return out


def row_solution(grism, x_ref, y_ref, sub_scale, S):
    """The per-row wavelength solution of a spatial scan -> (wl_a [S], wl_b [S]) in um and um / px: at bordered column
    coordinate u of bordered row y the first order carries lambda_y(u) = wl_a[y] + wl_b[y] u.  The grism's dispersion
    depends on the star's height, and row y is lit while the star is at the height y_s at which the trace crosses the
    row: with the row's centre in detector coordinates Y = y - 5 + sub_scale + 0.5, y_s solves
    get_trace(x_ref, y_s).wl_to_y(lambda_c) = Y at the centre lambda_c of the grism's [min_lambda, max_lambda] (fixed-point
    iteration; the trace is 1-2 px off the star's row and almost independent of y_s, so four steps converge far below
    1e-6 px).  Then wl_b = m_wl and wl_a = c_wl + m_wl (sub_scale - 5) of that trace: bordered u is detector column
    u - 5 + sub_scale.  `x_ref` is the exposure's nominal one (an observer does not know the jitter); the solution is a
    function of the detector row alone, so `y_ref` -- where the scan starts -- does not enter it.  Against the
    simulator's own bin positions over +-200 px the solution errs by 0.41 A (G141; G102 0.28 A): the term quadratic in
    x that a line omits, plus planning at the row's centre."""
    tr0 = grism.get_trace(x_ref, y_ref)
    coeff, wlsol = tr0.trace_coeff, tr0.wl_solution
    lam_c = 0.5 * (grism.min_lambda + grism.max_lambda)
    Y = np.arange(int(S), dtype=np.float64) - 5.0 + sub_scale + 0.5

    def lines(y_s):
        # _SpectrumTrace for an array of star heights: (m_t, c_t, m_wl, c_wl)
        m_t, c_t, m_w, c_w = grism_mod.wavelength_calibration_coeffs(x_ref, y_s, coeff, wlsol)
        xa, xb = x_ref + 10, x_ref + 20
        ya, yb = m_t * (xa - x_ref) + c_t + y_s, m_t * (xb - x_ref) + c_t + y_s
        wa = (m_w * np.sqrt((ya - y_s) ** 2 + (xa - x_ref) ** 2) + c_w) * 1e-4
        wb = (m_w * np.sqrt((yb - y_s) ** 2 + (xb - x_ref) ** 2) + c_w) * 1e-4
        m_wl = (wb - wa) / (xb - xa)
        return m_t, c_t, m_wl, wa - m_wl * xa

    y_s = Y.copy()
    for _ in range(4):
        m_t, c_t, m_wl, c_wl = lines(y_s)
        y_s = y_s + (Y - (m_t * ((lam_c - c_wl) / m_wl - x_ref) + c_t + y_s))
    m_t, c_t, m_wl, c_wl = lines(y_s)
    return c_wl + m_wl * (sub_scale - 5.0), m_wl * np.ones_like(Y)


def channel_weights(x_ref, edges, sub_scale, S):
    """[len(edges) - 1, S] fractional weights of the bordered columns for star-fixed channels: channel c covers
    [x* + edges[c], x* + edges[c + 1]) with x* = x_ref - sub_scale + 5, the star's bordered column; `edges` are offsets
    from the star in pixels."""
    edges = np.asarray(edges, dtype=float)
    x_star = x_ref - sub_scale + 5.0
    cols = np.arange(S, dtype=float)
    w = np.empty((len(edges) - 1, S))
    for c in range(len(edges) - 1):
        lo, hi = x_star + edges[c], x_star + edges[c + 1]
        w[c] = np.clip(np.minimum(cols + 1.0, hi) - np.maximum(cols, lo), 0.0, 1.0)
    return w


CHUNK_ROWS = 32            # rows of a chunk of a window (kExtractRows): partial sums are kept per chunk


def algorithmic_bytes(plan, S, R, read_bytes=4, crrej=False, channels=False, variance=False, optimal=False, profile=False,
                      deliver_profile=False, optimal_channels=False):
    """Bytes the extraction's kernels must move for `plan` on a frame of side S with R non-zero reads of `read_bytes`
    a sample: per pixel of product j's window the reads P_{j+1}, P_j, P_0 (P_0 once for j = 0 and for the last read),
    four coefficient planes, dark_{j+1} and dark_j (float32 each; dark_0 = 0 is not stored), the pixel flat and the
    master sky; the partial sums written and read once (2 float64 per chunk and column) and the result written.
    `crrej`: plus the mask kernel's -- per pixel of the mask rows the R + 1 reads, R dark planes, four coefficient planes
    and the pixel flat read once and the 2-byte flag word written; the word read again per window pixel; the chunks'
    counts (uint32 per chunk and column) written and read, and R + 1 counts written.  (The halo a tile re-reads and the
    neighbours of a flagged pixel are not algorithmic.)  `channels` (the plan carries them): plus k_extract_bins' -- per
    window pixel of the plan's column hull the same planes as above (and the flag word under `crrej`), four float32 flat
    planes when the flat is divided out, the row's wl_a / wl_b (2 float64 per row); the chunks' sums (2 C float64 per
    chunk) written and read once and channels [(R + 1) C] written.  `variance`: no plane is read for it -- plus the chunks'
    variance sums (a float64 per chunk and column; with `channels`, C float64 per chunk) written and read once and
    spectra_var, sky_var [(R + 1)(S + 1)] and, with `channels`, channels_var [(R + 1) C] written.  `optimal`: plus
    k_extract_optimal's -- per window pixel the planes k_extract_rows reads (the flag word under `crrej` too) once more, the
    chunks' sums (3 float64 per chunk and column) written and read once and optimal, optimal_var [2 (R + 1) S] written.
    (The halo a tile re-reads, 1.5 times the tile, is not algorithmic.)  `profile` (with `optimal`: a supplied
    profile): plus one float64 of the profile read per window pixel -- k_extract_optimal_fixed re-reads no halo.
    `deliver_profile` (with `optimal`): plus k_extract_profile's -- per window pixel the planes k_extract_rows reads (and the
    flag word) once more and a float64 of S1 written, zeros for the window of a last read that is not formed.
    `optimal_channels` (with `optimal` and `channels`): plus k_extract_bins_opt's -- the walk of the hull once more."""
    if optimal_channels and not (optimal and channels and plan.channels is not None):
        raise ValueError("algorithmic_bytes: optimal_channels belong to the optimal extraction and the channels")
    if (profile or deliver_profile) and not optimal:
        raise ValueError("algorithmic_bytes: profile and deliver_profile belong to the optimal extraction")
    total = 0
    hull = (plan.hull[1] - plan.hull[0]) if channels and plan.channels is not None else 0
    n_ch = plan.channels.n if hull or (channels and plan.channels is not None) else 0
    if crrej:
        lo, hi = plan.mask_rows
        total += (hi - lo) * S * ((R + 1) * read_bytes + 4 * R + 16 + 4 + 2) + (R + 1) * 4
    steps = plan.steps
    for p, (lo, hi) in enumerate(plan.row_windows[:R + 1]):
        if p == R and not steps & LAST_READ:
            if deliver_profile:
                total += max(int(hi) - int(lo), 0) * S * 8
            continue
        first = p == 0 or p == R                    # L_{r-1} = L_0 = 0: one read and one dark plane fewer
        per_pixel = (2 if first else 3) * read_bytes
        per_pixel += 16 if steps & LINEARISE else 0
        per_pixel += (4 if first else 8) if steps & DARK else 0
        per_pixel += 4 if steps & GAIN else 0
        per_pixel += 4 if steps & SKY else 0
        rows = int(hi) - int(lo)
        chunks = -(-rows // CHUNK_ROWS)
        total += rows * S * per_pixel + 2 * (2 * chunks * S * 8)
        if crrej:
            total += rows * S * 2 + 2 * (chunks * S * 4)
        if n_ch:
            total += rows * hull * (per_pixel + (2 if crrej else 0) + (16 if plan.channels.flat else 0))
            total += rows * 16 + 2 * (chunks * 2 * n_ch * 8)
        if variance:
            total += 2 * (chunks * S * 8) + 2 * (chunks * n_ch * 8)
        if optimal:
            total += rows * S * (per_pixel + (2 if crrej else 0)) + 2 * (3 * chunks * S * 8)
        if profile:
            total += rows * S * 8
        if deliver_profile:
            total += rows * S * (per_pixel + (2 if crrej else 0) + 8)
        if optimal_channels:
            # k_extract_bins' walk of the hull once more (with a supplied profile its float64 too), the columns' W from the
            # optimal scratch per chunk, the row groups' three sums written and read once
            total += rows * hull * (per_pixel + (2 if crrej else 0) + (16 if plan.channels.flat else 0) + (8 if profile else 0))
            total += rows * 16 + chunks * hull * 8 + 2 * (chunks * 3 * n_ch * 8)
    if optimal:
        total += 2 * (R + 1) * S * 8
    if optimal_channels:
        total += 2 * (R + 1) * n_ch * 8
    if variance:
        total += (R + 1) * (S + 1) * 8 + (R + 1) * n_ch * 8
    return total + (R + 1) * (S + 1) * 8 + (R + 1) * n_ch * 8


class Delivery(object):
    """What pipeline.run_pipelined sees of a context when an exposure's spectra are delivered: fetch_async / wait are the
    spectra calls, and wait hands `finish` (reads or None, spectra, sky) -- views of the slot's pinned buffers.  With
    `reads` the reads are copied too (both blocks follow the slot's kernels on its stream); without, they never leave
    the device."""

    def __init__(self, ctx, reads=False):
        self.ctx, self.reads = ctx, reads
        self.rejected = None      # n_rejected [R + 1] of the last wait (None: that slot extracts without rejection)
        self.channels = None      # channels [R + 1, C] of the last wait (None: that slot extracts without channels)
        self.variances = None     # (spectra_var, sky_var, channels_var or None) of the last wait (None: without variances)
        self.optimal = None       # (optimal, optimal_var) of the last wait (None: that slot extracts without them)
        self.channels_opt = None  # (channels_opt, channels_opt_var) of the last wait (None: that slot does not form them)
        self.profile_planes = None   # the planes S1 of the last wait (None: that slot does not deliver them)

    def upload(self, slot, desc):
        self.ctx.upload(slot, desc)

    def run(self, slot):
        self.ctx.run(slot)

    def fetch_async(self, slot):
        if self.reads:
            self.ctx.fetch_async(slot)
        self.ctx.fetch_spectra_async(slot)

    def wait(self, slot):
        reads = self.ctx.wait(slot) if self.reads else None
        spectra, sky = self.ctx.wait_spectra(slot)
        self.rejected = self.ctx.rejected(slot) if self.ctx.has_crrej(slot) else None
        self.channels = self.ctx.channels(slot) if self.ctx.has_channels(slot) else None
        self.variances = self.ctx.variances(slot) if self.ctx.has_variance(slot) else None
        self.optimal = self.ctx.optimal(slot) if self.ctx.has_optimal(slot) else None
        self.channels_opt = self.ctx.optimal_channels(slot) if self.ctx.has_optimal_channels(slot) else None
        # (a copy of its own, behind the settled run: wanted for the handful of exposures that form a visit's profile)
        self.profile_planes = self.ctx.profile_planes(slot) if self.ctx.delivers_profile(slot) else None
        return reads, spectra, sky


def save_npz(path, spectra, sky, exposure_index, plans, x_ref, y_ref, read_times, exp_start, rejected=None, channels=None,
             variances=None, optimal=None, optimal_profile_exposures=None, channels_opt=None):
    """The file --spectra / --spectra-only write: spectra [n, R + 1, S], sky [n, R + 1], exposure_index [n], row_lo /
    row_hi [n, R + 1], bg_cols [2], x_ref / y_ref [n], read_times [R], exp_start [n].  With `rejected` [n, R + 1] (the
    exposures were extracted with cosmic-ray rejection) also n_rejected [n, R + 1] -- flags in each product's window,
    (pixel, interval) pairs for the last-read product -- crrej_k and crrej_read_noise.  With `channels` [n, R + 1, C]
    (the exposures were binned into wavelength channels) also channels, channel_edges_um [C + 1], channel_flat and the
    rows' wavelength solutions wl_a / wl_b [n, S].  With `variances` = (spectra_var [n, R + 1, S], sky_var [n, R + 1],
    channels_var [n, R + 1, C] or None) (the exposures were extracted with variances) also spectra_var, sky_var,
    channels_var (with channels) and variance_read_noise.  With `optimal` = (optimal [n, R + 1, S], optimal_var
    [n, R + 1, S]) (the exposures were extracted optimally too) also optimal, optimal_var and optimal_half_width; with
    `optimal_profile_exposures` = N > 0 (their profiles were formed from the first N exposures of each group) also that;
    with `channels_opt` = (channels_opt, channels_opt_var [n, R + 1, C]) (the optimal channels) also those two."""
    n = len(exposure_index)
    more = {}
    if rejected is not None:
        cr = plans[0].crrej
        more = dict(n_rejected=np.asarray(rejected, dtype=np.uint32).reshape(n, -1), crrej_k=np.float64(cr.k),
                    crrej_read_noise=np.float64(cr.read_noise))
    if channels is not None:
        ch = plans[0].channels
        more.update(channels=np.asarray(channels, dtype=np.float64), channel_edges_um=ch.edges_um.copy(),
                    channel_flat=np.bool_(ch.flat),
                    wl_a=np.array([p.row_solution[0] for p in plans], dtype=np.float64).reshape(n, -1),
                    wl_b=np.array([p.row_solution[1] for p in plans], dtype=np.float64).reshape(n, -1))
    if variances is not None:
        more.update(spectra_var=np.asarray(variances[0], dtype=np.float64), sky_var=np.asarray(variances[1], dtype=np.float64),
                    variance_read_noise=np.float64(plans[0].variance.read_noise))
        if variances[2] is not None:
            more["channels_var"] = np.asarray(variances[2], dtype=np.float64)
    if optimal is not None:
        more.update(optimal=np.asarray(optimal[0], dtype=np.float64), optimal_var=np.asarray(optimal[1], dtype=np.float64),
                    optimal_half_width=np.int64(plans[0].optimal.half_width))
        if optimal_profile_exposures:
            more["optimal_profile_exposures"] = np.int64(optimal_profile_exposures)
        if channels_opt is not None:
            more.update(channels_opt=np.asarray(channels_opt[0], dtype=np.float64),
                        channels_opt_var=np.asarray(channels_opt[1], dtype=np.float64))
    np.savez(path, **more, spectra=np.asarray(spectra, dtype=np.float64), sky=np.asarray(sky, dtype=np.float64),
             exposure_index=np.asarray(exposure_index, dtype=np.int64),
             row_lo=np.array([p.row_lo for p in plans], dtype=np.int64).reshape(n, -1),
             row_hi=np.array([p.row_hi for p in plans], dtype=np.int64).reshape(n, -1),
             bg_cols=np.asarray(plans[0].bg_cols if plans else BG_COLS, dtype=np.int64),
             x_ref=np.asarray(x_ref, dtype=np.float64), y_ref=np.asarray(y_ref, dtype=np.float64),
             read_times=np.asarray(read_times, dtype=np.float64), exp_start=np.asarray(exp_start, dtype=np.float64))
