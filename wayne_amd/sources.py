"""Contaminating field stars: a neighbour's first-order spectrum on the same exposure (no reference counterpart).

A Contaminant is a second star at a fixed detector offset (dx, dy) px from the target, with its own spectrum on its own
wavelength grid, already cropped to the grism's band.  The device throws its electrons with the target's (wayne_hip.h
wayne_exposure_set_sources): jitter and scan are shared, it does not transit, it adds no cosmic rays of its own, and
its random streams are keyed by `tag` (wayne_source_seed).

Brightness is given as `flux_ratio`: the ratio of the contaminant's expected detected electrons to the target's, i.e.
of their sensitivity-weighted band integrals  sum(flux * sensitivity(wl) * bin width)  over the grism's range, each on
its own grid -- what "a companion 1.5 mag fainter in the grism band" means (flux_ratio = 10 ** (-1.5 / 2.5)).

Not modelled: zeroth and second grism orders; a contaminant in the direct image; a contaminant that varies or eclipses;
offsets that change within an exposure; replay mode (rng_mode RNG_REPLAY reproduces the reference, which has no second
star).
"""
import math
import os

import numpy as np

from . import tools

MAX_CONTAMINANTS = 8     # wayne_hip.h WAYNE_MAX_SOURCES


class ContaminantConfigError(ValueError):
    pass


class Contaminant(object):
    """One field star: offset (dx, dy) px from the target's x_ref / y_ref, its spectrum (wl in micron, flux in the
    target's flux units and scaling, cropped to the grism's band) and its stream tag (>= 1, unique in the visit)."""

    __slots__ = ("dx", "dy", "wl", "flux", "tag", "flux_ratio")

    def __init__(self, dx, dy, wl, flux, tag, flux_ratio=None):
        self.dx, self.dy = float(dx), float(dy)
        self.wl = np.ascontiguousarray(wl, dtype=np.float64)
        self.flux = np.ascontiguousarray(flux, dtype=np.float64)
        self.tag = int(tag)
        self.flux_ratio = None if flux_ratio is None else float(flux_ratio)
        if self.wl.shape != self.flux.shape or self.wl.ndim != 1 or self.wl.size < 2:
            raise ValueError("contaminant: wl and flux must be 1-D arrays of the same length >= 2")
        if self.tag < 1:
            raise ValueError("contaminant: tag must be >= 1 (0 is the target's)")
        if not (math.isfinite(self.dx) and math.isfinite(self.dy)):
            raise ValueError("contaminant: offset must be finite")

    def __repr__(self):
        return "Contaminant(dx=%r, dy=%r, tag=%d, W=%d)" % (self.dx, self.dy, self.tag, self.wl.size)

    def digest_bytes(self):
        """What identifies the source in a descriptor digest (visit.descriptor_digest)."""
        return (np.array([self.tag], dtype=np.int64).tobytes() + np.array([self.dx, self.dy], dtype=np.float64).tobytes()
                + self.wl.tobytes() + self.flux.tobytes())

    @classmethod
    def from_config(cls, entry, tag, grism, target_wl, target_flux, base_dir="."):
        """A `contaminants:` entry of the YAML (run_visit) -> Contaminant.  `target_wl` / `target_flux`: the target's
        spectrum as the exposures get it (flux_scale applied), before the crop to the grism's band."""
        if not isinstance(entry, dict):
            raise ContaminantConfigError("contaminant %d: expected a mapping with dx, dy, flux_ratio and a spectrum" % tag)
        for key in ("dx", "dy"):
            if entry.get(key) is None:
                raise ContaminantConfigError("contaminant %d: missing `%s`" % (tag, key))
        try:
            dx, dy = float(entry["dx"]), float(entry["dy"])
        except (TypeError, ValueError):
            raise ContaminantConfigError("contaminant %d: dx / dy must be numbers" % tag)
        if not (math.isfinite(dx) and math.isfinite(dy)):
            raise ContaminantConfigError("contaminant %d: dx / dy must be finite" % tag)
        ratio = entry.get("flux_ratio")
        try:
            ratio = float(ratio)
        except (TypeError, ValueError):
            raise ContaminantConfigError("contaminant %d: `flux_ratio` must be a number > 0" % tag)
        if not (math.isfinite(ratio) and ratio > 0):
            raise ContaminantConfigError("contaminant %d: `flux_ratio` must be finite and > 0, got %r" % (tag, ratio))
        lo, hi = grism.wl_limits[0], grism.wl_limits[-1]
        t_wl, t_flux = tools.crop_spectrum(lo, hi, np.asarray(target_wl, dtype=float), np.asarray(target_flux, dtype=float))
        spectrum_file = entry.get("spectrum_file")
        temperature = entry.get("temperature")
        if spectrum_file:
            p = spectrum_file if os.path.isabs(spectrum_file) else os.path.join(base_dir, spectrum_file)
            if not os.path.exists(p):
                raise ContaminantConfigError("contaminant %d: spectrum_file %s not found" % (tag, p))
            wl, flux = tools.load_pheonix_stellar_grid_fits(p)
            wl, flux = tools.crop_spectrum(lo, hi, wl, flux)
        elif temperature is not None:
            try:
                T = float(temperature)
            except (TypeError, ValueError):
                raise ContaminantConfigError("contaminant %d: `temperature` must be a number" % tag)
            if not (math.isfinite(T) and T > 0):
                raise ContaminantConfigError("contaminant %d: `temperature` must be finite and > 0" % tag)
            wl = t_wl.copy()                   # a black body on the target's grid
            flux = tools.blackbody_lambda(wl, T)
        else:
            raise ContaminantConfigError("contaminant %d: give a `spectrum_file` or a `temperature`" % tag)
        if wl.size < 2:
            raise ContaminantConfigError("contaminant %d: fewer than 2 wavelengths inside the grism's band" % tag)
        flux = scale_to_ratio(grism, wl, flux, t_wl, t_flux, ratio)
        return cls(dx, dy, wl, flux, tag, flux_ratio=ratio)


def band_integral(grism, wl, flux):
    """sum(flux * sensitivity(wl) * bin width) on the grid `wl`: the expected detected electrons per unit time up to a
    common factor (the device's counts chain: k_prep_wl / k_prep_sub)."""
    sens_wl, sens_val = grism.calibration.sensitivity(grism.name)
    wl = np.asarray(wl, dtype=float)
    return float(np.sum(np.asarray(flux, dtype=float) * np.interp(wl, sens_wl, sens_val) * tools.bin_centers_to_widths(wl)))


def scale_to_ratio(grism, wl, flux, target_wl, target_flux, ratio):
    """`flux` scaled so that its band integral is `ratio` times the target's."""
    mine, theirs = band_integral(grism, wl, flux), band_integral(grism, target_wl, target_flux)
    if not (mine > 0 and theirs > 0 and math.isfinite(mine) and math.isfinite(theirs)):
        raise ContaminantConfigError("contaminant: a spectrum with no electrons in the grism's band cannot be scaled")
    return np.asarray(flux, dtype=float) * (ratio * theirs / mine)


def from_config(entries, grism, target_wl, target_flux, base_dir="."):
    """The YAML's `contaminants:` list -> [Contaminant]; tags are the 1-based list positions."""
    if entries is None:
        return []
    if not isinstance(entries, (list, tuple)):
        raise ContaminantConfigError("`contaminants` must be a list")
    if len(entries) > MAX_CONTAMINANTS:
        raise ContaminantConfigError("at most %d contaminants, got %d" % (MAX_CONTAMINANTS, len(entries)))
    return [Contaminant.from_config(e, i + 1, grism, target_wl, target_flux, base_dir) for i, e in enumerate(entries)]
