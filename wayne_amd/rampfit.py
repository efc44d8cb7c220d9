"""The ramp fit of an exposure, beside the exposure (k_ramp_fit; include/wayne_hip.h, "the ramp fit").

`ramp_fit=True | RampFit(...)` on ExposureGenerator.scanning_frame / staring_frame / build_descriptor asks for it;
Context.upload applies it (wayne_exposure_set_rampfit) and every run of the slot then fits every light-sensitive pixel's
up-the-ramp samples with a line, near the end of its back half: samples from the first saturated one on are dropped, an
upward jump (a cosmic ray) is cut out of the ramp, and the intervals that remain are fitted by generalised least squares
with the covariance of differences that share a read.  The device delivers three planes [S, S]:

    rate   float64, e-/s        var   float64, (e-/s)^2        word   uint32 = K << 16 | jump

K the usable samples, bit j of `jump` a removed interval.  Derived here, on the host: `nsamp = K - popcount(jump)`,
`time = sum of the dt_j that were fitted` and the data-quality value `dq`: 256 where K < R (full well), 8192 where a jump
was cut out (cosmic ray rejected) -- the instrument pipeline's bits, quoted without the handbook at hand.

This is the product of a STARING exposure.  In a scan the star crossing a pixel is a jump: with the jump test on, the
scan's trace is flagged as cosmic rays (as the instrument pipeline's flt does with scans); the extraction stays the
scan product.

Here: the option itself, the derived planes, the delivery of the planes in an exposure loop (pipeline.run_pipelined)
and their FITS file.
"""
import os

import numpy as np

from . import _lib, fitsio

X_LINEARISE, X_DARK, X_GAIN = 1, 2, 4      # WAYNE_X_*
DQ_SATURATED, DQ_JUMP = 256, 8192


class RampFit(object):
    """The ramp fit of an exposure (wayne_rampfit_desc): `read_noise`, the noise of a difference of two reads in
    electrons (finite, > 0; the meaning and default of extraction.Variances.read_noise); `k`, the jump threshold in
    sigma (finite, >= 0; 0 switches the jump test off); `saturation_dn`, the raw value from which on a sample and every
    later one are dropped (finite, > 0; the default lies below the 78000 DN clip and the uint16 ceiling); `linearise` /
    `dark`: the extraction's steps of the same names.  The gain step is always on: the fit is in electrons."""

    def __init__(self, read_noise=20.0, k=5.0, saturation_dn=65000.0, linearise=True, dark=True):
        read_noise, k, saturation_dn = float(read_noise), float(k), float(saturation_dn)
        if not (np.isfinite(read_noise) and read_noise > 0.0):
            raise ValueError("RampFit: read_noise must be finite and > 0")
        if not (np.isfinite(k) and k >= 0.0):
            raise ValueError("RampFit: k must be finite and >= 0")
        if not (np.isfinite(saturation_dn) and saturation_dn > 0.0):
            raise ValueError("RampFit: saturation_dn must be finite and > 0")
        self.read_noise, self.k, self.saturation_dn = read_noise, k, saturation_dn
        self.linearise, self.dark = bool(linearise), bool(dark)

    @property
    def steps(self):
        return X_GAIN | (X_LINEARISE if self.linearise else 0) | (X_DARK if self.dark else 0)

    def desc(self):
        d = _lib.RampFitDesc()
        d.steps, d.read_noise_e, d.k_jump, d.saturation_dn = self.steps, self.read_noise, self.k, self.saturation_dn
        return d

    def __repr__(self):
        return "RampFit(read_noise=%r, k=%r, saturation_dn=%r, linearise=%r, dark=%r)" % (
            self.read_noise, self.k, self.saturation_dn, self.linearise, self.dark)


def as_ramp_fit(ramp_fit):
    """`ramp_fit=` -> a RampFit or None: None and False are off, True the defaults; a number is the jump threshold."""
    if ramp_fit is None or ramp_fit is False:
        return None
    if ramp_fit is True:
        return RampFit()
    if isinstance(ramp_fit, RampFit):
        return ramp_fit
    if isinstance(ramp_fit, (int, float)):
        return RampFit(k=ramp_fit)
    raise TypeError("ramp_fit: None, True, a jump threshold or a rampfit.RampFit, not %r" % (ramp_fit,))


def derive(word, read_dt):
    """A word plane and the exposure's read intervals -> (dq uint16, nsamp uint16, time float64), the planes' shape."""
    word = np.asarray(word, dtype=np.uint32)
    read_dt = np.asarray(read_dt, dtype=np.float64)
    R = read_dt.size
    K, jump = word >> np.uint32(16), word & np.uint32(0xFFFF)
    dq = np.where(K < R, DQ_SATURATED, 0) | np.where(jump != 0, DQ_JUMP, 0)
    nsamp = np.zeros(word.shape, dtype=np.uint16)
    time = np.zeros(word.shape, dtype=np.float64)
    for j in range(R):
        fitted = (K > j) & (((jump >> np.uint32(j)) & np.uint32(1)) == 0)
        nsamp += fitted
        time += np.where(fitted, read_dt[j], 0.0)
    return dq.astype(np.uint16), nsamp, time


def fill_exposure(frame, planes, read_dt):
    """The planes Context.rampfit returned -> Exposure.rate / .rate_var / .rate_word and the derived .rate_dq /
    .rate_nsamp / .rate_time."""
    frame.rate, frame.rate_var, frame.rate_word = planes
    frame.rate_dq, frame.rate_nsamp, frame.rate_time = derive(frame.rate_word, read_dt)
    return frame


class RampFitDelivery(object):
    """A context (or another delivery: extraction.Delivery, expected.ExpectedDelivery) for pipeline.run_pipelined whose
    wait(slot) also brings the slot's ramp fit back: `ramp_fit` holds (rate, var, word) -- arrays of the caller's own --
    or None for a slot that did not ask, until the next wait.  The planes are fetched behind the settled run by a call
    of their own (Context.rampfit).  Everything else is the inner object's."""

    def __init__(self, ctx, inner=None):
        self._ctx = ctx
        self._inner = inner if inner is not None else ctx
        self.ramp_fit = None

    def upload(self, slot, desc):
        self._inner.upload(slot, desc)

    def run(self, slot):
        self._inner.run(slot)

    def fetch_async(self, slot):
        self._inner.fetch_async(slot)

    def wait(self, slot):
        got = self._inner.wait(slot)
        self.ramp_fit = self._ctx.rampfit(slot) if self._ctx.has_rampfit(slot) else None
        return got

    def __getattr__(self, name):
        return getattr(self._inner, name)


def refuse_combinations(ramp_fit, resume=False, device_fits=False, spectra_only=False):
    """The visit-level options the ramp fit is not delivered with: ValueError before anything starts."""
    if as_ramp_fit(ramp_fit) is None:
        return
    for on, what, why in ((resume, "resume", "an exposure a resumed visit skips has no rate image"),
                          (device_fits, "device_fits", "the files are written from the slots' pinned mirrors, which hold no rate image"),
                          (spectra_only, "spectra_only", "no exposure files are written to put the _rate files beside")):
        if on:
            raise ValueError("ramp_fit: not together with %s (%s)" % (what, why))


def rate_filename(raw_filename):
    """NNNN_raw.fits -> NNNN_rate.fits."""
    root, ext = os.path.splitext(raw_filename)
    return (root[:-4] if root.endswith("_raw") else root) + "_rate" + ext


def write_fits(path, exposure, ramp_fit):
    """The rate image of `exposure` (which carries the planes: fill_exposure) as a FITS file: the raw file's primary header
    plus RFRN, RFK and RFSAT, then the image HDUs SCI (BITPIX -32, e-/s), ERR (-32, sqrt var), DQ (16), SAMP (16) and TIME
    (-32, s), EXTVER 1 each."""
    fit = as_ramp_fit(ramp_fit)
    if fit is None or getattr(exposure, "rate", None) is None:
        raise ValueError("write_fits: the exposure carries no ramp fit")
    rate, var = exposure.rate, exposure.rate_var
    dq, nsamp, time = exposure.rate_dq, exposure.rate_nsamp, exposure.rate_time
    cards = list(exposure.generate_science_header().cards)
    cards += [("RFRN", fit.read_noise, "ramp fit: read noise of a difference (e-)"),
              ("RFK", fit.k, "ramp fit: jump threshold (sigma; 0: off)"),
              ("RFSAT", fit.saturation_dn, "ramp fit: saturation (DN)")]
    hdus = [fitsio.HDU(fitsio.Header(cards), None)]
    for name, data, unit in (("SCI", np.asarray(rate, dtype=np.float32), "ELECTRONS/S"),
                             ("ERR", np.sqrt(np.asarray(var, dtype=np.float64)).astype(np.float32), "ELECTRONS/S"),
                             ("DQ", np.asarray(dq).astype(np.int16), "UNITLESS"),
                             ("SAMP", np.asarray(nsamp).astype(np.int16), "SAMPLES"),
                             ("TIME", np.asarray(time, dtype=np.float32), "SECONDS")):
        hdus.append(fitsio.HDU(fitsio.Header([("EXTVER", 1, "extension version"), ("BUNIT", unit, "")]), data, name=name))
    fitsio.write(path, hdus)
    return path
