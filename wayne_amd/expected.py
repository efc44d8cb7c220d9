"""The noise-free expected image of an exposure, beside the exposure (k_expect; include/wayne_hip.h, "the noise-free
expected image").

`expected="counts" | "mean"` on ExposureGenerator.scanning_frame / staring_frame / build_descriptor asks for it;
Context.upload applies it (wayne_exposure_set_expected) and every run of the slot then renders E [R, S, S] float64 --
electrons per read interval, the 5-pixel border zero -- at the very end of its back half:

    E_r[y + 5, x + 5] = sum_s sum_{k: read(k) = r} f_{s,k}(y, x) sum_w ( n_h a(x; xs, sigma_h) a(y; ys, sigma_h)
                                                                     + n_l a(x; xs, sigma_l) a(y; ys, sigma_l) )
    a(p; c, sigma)    = Phi((p + 1 - c) / sigma) - Phi((p - c) / sigma)   for 1 <= p <= N - 1, else 0

"counts": (n_h, n_l) are the bin's wide and narrow electrons as this run drew them -- E is the exact conditional
expectation of the thrower's accumulators; "mean": the counts chain before the draw, shared out by the PSF ratio -- the
unconditional expectation (up to the truncation of the wide count, < 1 electron per bin and sub-sample, and with
stellar noise off the rounding of the counts).  NOT in E: sky, cosmic rays, dark current, the gaussian-noise stage, gain,
non-linearity, charge traps: it is the truth of the thrower stage, not a noise-free read.

Here: the delivery of the planes in an exposure loop (pipeline.run_pipelined) and their FITS file.
"""
import os

import numpy as np

from . import _lib, fitsio

MODES = tuple(_lib.EXPECT_MODES)


class ExpectedDelivery(object):
    """A context (or another delivery: extraction.Delivery, fits_delivery.FitsDelivery) for pipeline.run_pipelined whose
    wait(slot) also brings the slot's expected image back: `expected` holds it -- an array of the caller's own
    [R, S, S], or None for a slot that did not ask -- until the next wait.  The planes are fetched behind the settled
    run by a call of their own (Context.expected), as the profile planes of the optimal extraction are.  Everything
    else is the inner object's."""

    def __init__(self, ctx, inner=None):
        self._ctx = ctx
        self._inner = inner if inner is not None else ctx
        self.expected = None

    def upload(self, slot, desc):
        self._inner.upload(slot, desc)

    def run(self, slot):
        self._inner.run(slot)

    def fetch_async(self, slot):
        self._inner.fetch_async(slot)

    def wait(self, slot):
        got = self._inner.wait(slot)
        self.expected = self._ctx.expected(slot) if self._ctx.has_expected(slot) else None
        return got

    def __getattr__(self, name):
        return getattr(self._inner, name)


def refuse_combinations(expected, resume=False, device_fits=False, spectra=False, spectra_only=False):
    """The visit-level options the expected image is not delivered with: ValueError before anything starts."""
    if not _lib.expected_mode(expected):
        return
    for on, what, why in ((resume, "resume", "an exposure a resumed visit skips has no expected image"),
                          (device_fits, "device_fits", "the files are written from the slots' pinned mirrors, which hold no expected image"),
                          (spectra_only, "spectra_only", "no exposure files are written to put the _exp files beside"),
                          (spectra, "spectra", "the expected image is not fed through the extraction")):
        if on:
            raise ValueError("expected: not together with %s (%s)" % (what, why))


def exp_filename(raw_filename):
    """NNNN_raw.fits -> NNNN_exp.fits."""
    root, ext = os.path.splitext(raw_filename)
    return (root[:-4] if root.endswith("_raw") else root) + "_exp" + ext


def write_fits(path, exposure, planes, mode):
    """The expected image of `exposure` as a FITS file: the raw file's primary header plus EXPMODE, then R image HDUs
    EXPECT, EXTVER 1 .. R (BITPIX -64), read interval 0 first."""
    planes = np.asarray(planes, dtype=np.float64)
    cards = list(exposure.generate_science_header().cards)
    cards.append(("EXPMODE", _lib.EXPECT_NAMES[_lib.expected_mode(mode)], "expected image: counts (conditional) or mean"))
    hdus = [fitsio.HDU(fitsio.Header(cards), None)]
    for r in range(planes.shape[0]):
        ext = fitsio.Header([("EXTVER", r + 1, "read interval"), ("BUNIT", "ELECTRONS", "expected per read interval")])
        hdus.append(fitsio.HDU(ext, planes[r], name="EXPECT"))
    fitsio.write(path, hdus)
    return path
