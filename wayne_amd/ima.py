"""The calibrated reads of an exposure -- the SCI, ERR and DQ arrays of the instrument pipeline's intermediate file,
`_ima.fits` -- beside the exposure (k_ima; include/wayne_hip.h, "the calibrated reads").

`ima=True | "rate" | "counts" | Ima(...)` on ExposureGenerator.scanning_frame / staring_frame / build_descriptor asks for
them; Context.upload applies it (wayne_exposure_set_ima) and every run of the slot then forms, behind its reads, for
every read k: the electrons accumulated since the zero read (the zero read subtracted, linearised, dark-subtracted, times
the gain), or that over the read's time; their error sqrt(max(e_k, 0) + rn^2 q^2); and a data-quality value -- 256 for a
read at or behind the first one at saturation_dn, 8192 for a read behind an interval the slot's ramp fit (ramp_fit=) cut
out as a cosmic ray.  The device writes them as the bytes of the file: one payload, the last read first,

    imset f = 0 .. R (read k = R - f):  SCI_k  S*S big-endian float32, zeros to sci_stride
                                        ERR_k  the same
                                        DQ_k   S*S big-endian int16, zeros to dq_stride

which `write_fits` hands to the file between cached header blocks without a pass over the samples.

This is what a SCAN observer with a reduction of their own starts from: they difference consecutive reads of the file.
With a ramp fit on the same exposure and its jump test on, the scan's trace itself carries 8192, as in the instrument's
ima: the star crossing a pixel is a jump.  Not in it: reference-pixel values and a bias-level correction, the zero-read
signal correction, flat-fielding, the direct image.

Here: the option itself, the payload's layout and views, the delivery of the payload in an exposure loop
(pipeline.run_pipelined) and the FITS file.
"""
import collections
import os

import numpy as np

from . import _lib, fitsio

X_LINEARISE, X_DARK, X_GAIN = 1, 2, 4      # WAYNE_X_*
RATE, COUNTS = 1, 2                        # WAYNE_IMA_*
UNITS = {"rate": RATE, "counts": COUNTS}
BUNIT = {"rate": "ELECTRONS/S", "counts": "ELECTRONS"}
DQ_SATURATED, DQ_JUMP = 256, 8192
MAX_READS = 16

Layout = collections.namedtuple("Layout", "S R sci_stride dq_stride imset_stride nbytes")


def _pad(b):
    return (b + fitsio.BLOCK - 1) // fitsio.BLOCK * fitsio.BLOCK


def layout(S, R):
    """The payload's Layout for a frame of side S with R read intervals (wayne_ima_layout's arithmetic)."""
    S, R = int(S), int(R)
    if S < 12 or S % 2 or not 1 <= R < MAX_READS:
        raise ValueError("ima: no layout for side %d with %d read intervals" % (S, R))
    n = S * S
    sci, dq = _pad(4 * n), _pad(2 * n)
    return Layout(S, R, sci, dq, 2 * sci + dq, (R + 1) * (2 * sci + dq))


class Ima(object):
    """The calibrated reads of an exposure (wayne_ima_desc): `units`, "rate" (e-/s) or "counts" (e-); `read_noise`, the
    noise of a difference of two reads in electrons (finite, > 0; the meaning and default of
    extraction.Variances.read_noise); `saturation_dn`, the raw value from which on a read and every later one are flagged
    (finite, > 0; the ramp fit's default); `linearise` / `dark`: the extraction's steps of the same names.  The gain step
    is always on: the reads are in electrons."""

    def __init__(self, units="rate", read_noise=20.0, saturation_dn=65000.0, linearise=True, dark=True):
        if units not in UNITS:
            raise ValueError("Ima: units must be 'rate' or 'counts', not %r" % (units,))
        read_noise, saturation_dn = float(read_noise), float(saturation_dn)
        if not (np.isfinite(read_noise) and read_noise > 0.0):
            raise ValueError("Ima: read_noise must be finite and > 0")
        if not (np.isfinite(saturation_dn) and saturation_dn > 0.0):
            raise ValueError("Ima: saturation_dn must be finite and > 0")
        self.units, self.read_noise, self.saturation_dn = units, read_noise, saturation_dn
        self.linearise, self.dark = bool(linearise), bool(dark)

    @property
    def steps(self):
        return X_GAIN | (X_LINEARISE if self.linearise else 0) | (X_DARK if self.dark else 0)

    def desc(self):
        d = _lib.ImaDesc()
        d.steps, d.units, d.read_noise_e, d.saturation_dn = self.steps, UNITS[self.units], self.read_noise, self.saturation_dn
        return d

    def __repr__(self):
        return "Ima(units=%r, read_noise=%r, saturation_dn=%r, linearise=%r, dark=%r)" % (
            self.units, self.read_noise, self.saturation_dn, self.linearise, self.dark)


def as_ima(ima):
    """`ima=` -> an Ima or None: None and False are off, True the defaults; "rate" / "counts" the defaults in that unit."""
    if ima is None or ima is False:
        return None
    if ima is True:
        return Ima()
    if isinstance(ima, Ima):
        return ima
    if isinstance(ima, str):
        return Ima(units=ima)
    raise TypeError("ima: None, True, 'rate', 'counts' or an ima.Ima, not %r" % (ima,))


class Payload(object):
    """The calibrated reads of one exposure: `bytes`, the payload as one uint8 array (Layout.nbytes of it), `layout` and
    the option `ima` it was formed with.  sci(k) / err(k) [S, S] ">f4" and dq(k) [S, S] ">i2" are views of it, no copy;
    piece(k, which) is a section with its padding, as the file holds it."""

    def __init__(self, data, lay, ima=None):
        data = np.asarray(data)
        if data.dtype != np.uint8 or data.ndim != 1 or data.size != lay.nbytes:
            raise ValueError("ima payload: %d bytes of uint8 are expected" % lay.nbytes)
        self.bytes, self.layout, self.ima = data, lay, ima

    def _offset(self, k, which):
        lay = self.layout
        if not 0 <= k <= lay.R:
            raise IndexError("read %d of %d" % (k, lay.R + 1))
        return (lay.R - k) * lay.imset_stride + {"SCI": 0, "ERR": lay.sci_stride, "DQ": 2 * lay.sci_stride}[which]

    def _plane(self, k, which, dtype):
        S = self.layout.S
        at = self._offset(k, which)
        return self.bytes[at:at + S * S * np.dtype(dtype).itemsize].view(dtype).reshape(S, S)

    def sci(self, k):
        return self._plane(k, "SCI", ">f4")

    def err(self, k):
        return self._plane(k, "ERR", ">f4")

    def dq(self, k):
        return self._plane(k, "DQ", ">i2")

    def piece(self, k, which):
        at = self._offset(k, which)
        return self.bytes[at:at + (self.layout.dq_stride if which == "DQ" else self.layout.sci_stride)]


class ImaDelivery(object):
    """A context (or another delivery: extraction.Delivery, expected.ExpectedDelivery, rampfit.RampFitDelivery) for
    pipeline.run_pipelined whose wait(slot) also brings the slot's calibrated reads back: `ima` holds a Payload -- bytes of
    the caller's own -- or None for a slot that did not ask, until the next wait.  The payload is fetched behind the
    settled run by a call of its own (Context.ima).  Everything else is the inner object's."""

    def __init__(self, ctx, inner=None):
        self._ctx = ctx
        self._inner = inner if inner is not None else ctx
        self.ima = None

    def upload(self, slot, desc):
        self._inner.upload(slot, desc)

    def run(self, slot):
        self._inner.run(slot)

    def fetch_async(self, slot):
        self._inner.fetch_async(slot)

    def wait(self, slot):
        got = self._inner.wait(slot)
        self.ima = self._ctx.ima(slot) if self._ctx.has_ima(slot) else None
        return got

    def __getattr__(self, name):
        return getattr(self._inner, name)


def refuse_combinations(ima, resume=False, device_fits=False, spectra_only=False):
    """The visit-level options the calibrated reads are not delivered with: ValueError before anything starts."""
    if as_ima(ima) is None:
        return
    for on, what, why in ((resume, "resume", "an exposure a resumed visit skips has no calibrated reads"),
                          (device_fits, "device_fits", "the files are written from the slots' pinned mirrors, which hold no calibrated reads"),
                          (spectra_only, "spectra_only", "no exposure files are written to put the _ima files beside")):
        if on:
            raise ValueError("ima: not together with %s (%s)" % (what, why))


def ima_filename(raw_filename):
    """NNNN_raw.fits -> NNNN_ima.fits."""
    root, ext = os.path.splitext(raw_filename)
    return (root[:-4] if root.endswith("_raw") else root) + "_ima" + ext


def write_fits(path, exposure, payload=None):
    """The calibrated reads of `exposure` (`payload`, by default the Payload it carries as `ima`) as a FITS file laid out
    like the raw file: the raw file's primary header plus IMAUNIT, IMARN, IMASAT, IMALIN and IMADARK, then for each read in
    reverse time order SCI (BITPIX -32, SAMPNUM / SAMPTIME / DELTATIM / CRPIX1 as in the raw file), ERR (-32), DQ (16)
    and the data-less SAMP and TIME with PIXVALUE, EXTVER counted as in the raw file: read r sits at HDU
    1 + 5 (NSAMP - 1 - r).  The data sections are views of the payload between cached header blocks."""
    payload = payload if payload is not None else getattr(exposure, "ima", None)
    if payload is None:
        raise ValueError("write_fits: the exposure carries no calibrated reads")
    opt, lay = payload.ima if payload.ima is not None else Ima(), payload.layout
    headers = [h for _, h in exposure.reads] if exposure.reads else [s[1] for s in exposure.stored]
    n = lay.R + 1
    if len(headers) != n:
        raise ValueError("write_fits: the payload holds %d reads, the exposure %d" % (n, len(headers)))
    cards = list(exposure.generate_science_header().cards)
    cards += [("IMAUNIT", opt.units.upper(), "calibrated reads: RATE (e-/s) or COUNTS (e-)"),
              ("IMARN", opt.read_noise, "calibrated reads: read noise of a difference (e-)"),
              ("IMASAT", opt.saturation_dn, "calibrated reads: saturation (DN)"),
              ("IMALIN", opt.linearise, "calibrated reads: linearised (T/F)"),
              ("IMADARK", opt.dark, "calibrated reads: dark subtracted (T/F)")]
    pieces = [fitsio._image_hdu_parts(None, cards, primary=True)[0]]
    t, times = 0.0, []
    for h in headers:                      # t_k: the read intervals summed in ascending order
        t = t + float(h.get("DELTATIM", 0.0))
        times.append(t)
    shape, unit = (lay.S, lay.S), BUNIT[opt.units]
    for i in range(n):
        k = n - 1 - i
        h = headers[k]
        sampt, delt, crpix = float(h.get("SAMPTIME", 0.0)), float(h.get("DELTATIM", 0.0)), h.get("CRPIX1", 0)
        ver = i + 1
        sci = [("SAMPNUM", k, ""), ("SAMPTIME", sampt, "s"), ("DELTATIM", delt, "s"), ("CRPIX1", crpix, ""),
               ("EXTVER", ver, ""), ("BUNIT", unit, "")]
        pieces.append(fitsio.cached_header_block(("IMA-SCI", shape, k, sampt, delt, type(crpix), crpix, ver, unit), sci,
                                                 data_shape=shape, dtype_code="f4", name="SCI"))
        pieces.append(payload.piece(k, "SCI"))
        pieces.append(fitsio.cached_header_block(("IMA-ERR", shape, ver, unit), [("EXTVER", ver, ""), ("BUNIT", unit, "")],
                                                 data_shape=shape, dtype_code="f4", name="ERR"))
        pieces.append(payload.piece(k, "ERR"))
        pieces.append(fitsio.cached_header_block(("IMA-DQ", shape, ver), [("EXTVER", ver, ""), ("BUNIT", "UNITLESS", "")],
                                                 data_shape=shape, dtype_code="i2", name="DQ"))
        pieces.append(payload.piece(k, "DQ"))
        samp = 1 if k > 0 else 0
        pieces.append(fitsio.cached_header_block(("IMA-SAMP", ver, samp), [("EXTVER", ver, ""), ("PIXVALUE", samp, "values of pixels in constant array"),
                                                                            ("BUNIT", "SAMPLES", "")], name="SAMP"))
        pieces.append(fitsio.cached_header_block(("IMA-TIME", ver, times[k]), [("EXTVER", ver, ""), ("PIXVALUE", times[k], "values of pixels in constant array"),
                                                                               ("BUNIT", "SECONDS", "")], name="TIME"))
    fitsio.write_pieces(path, pieces)
    return path
