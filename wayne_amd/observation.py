"""Observation: a whole visit of exposures.

Same class and `setup_*` / `run_observation` methods as the reference's
wayne/observation.py:24-538, with plain floats (days, micron, seconds, px/s,
counts/s) instead of astropy / quantities objects and a small `Planet` record
instead of an exodata object.  What changed underneath:

  * light curves: the reference calls pylightcurve once per wavelength element
    per exposure (observation.py:349-355); here the K x W depth matrix of an
    exposure is computed on the GPU from the orbit (wayne_amd/lightcurve.py,
    k_lightcurve);
  * exposures are independent (counter-based RNG), so `run_observation` can
    take a (rank, world) pair and generate only its round-robin share.
"""
import os

import numpy as np

from . import lightcurve, tools
from .exposure_generator import ExposureGenerator
from .trend_generators import visit_trends
from .visit_planner import VisitPlanner

R_SUN_AU = 0.00465047      # solar radius in au


class Planet(object):
    """Orbital elements needed for the light curve (what the reference reads off an
    exodata Planet, observation.py:317-324)."""

    def __init__(self, name="planet", period=None, sma_au=None, stellar_radius_rsun=None, inclination=None,
                 eccentricity=0.0, periastron=0.0, transittime=None, rp_over_rs=None, star_temperature=None,
                 ra_deg=None, dec_deg=None):
        self.name = name
        self.ra_deg, self.dec_deg = ra_deg, dec_deg        # target coordinates (J2000, degrees) for JD -> HJD
        self.P, self.a, self.Rs = period, sma_au, stellar_radius_rsun
        self.i, self.e, self.periastron = inclination, eccentricity, periastron
        self.transittime = transittime
        self.rp_over_rs = rp_over_rs
        self.star_temperature = star_temperature

    @property
    def sma_over_rs(self):
        return self.a / (self.Rs * R_SUN_AU)


class Observation(object):
    def __init__(self, outdir="", calibration=None, device=0, seed=0):
        self.scanning = True
        self.outdir = outdir
        self.calibration = calibration
        self.device, self.seed = device, seed
        self._visit_trend = False
        self.ssv_gen = None
        self.noise_mean = self.noise_std = False
        # extra keywords for scanning_frame / staring_frame (rng_mode, out_dtype, exact_samplers, reference_quirks).
        # The visit driver asks for float32 reads: the FITS writer stores them as the reference's float64 SCI images
        # (BITPIX -64) either way, and a full-array exposure is 67 MB instead of 134 MB to bring over PCIe;
        # frame_options["out_dtype"] = np.float64 (CLI: --float64-reads) keeps the float64 arithmetic to the file;
        # np.uint16 (CLI: --uint16-reads) makes the reads and the files' SCI images 16-bit unsigned DN (BITPIX 16).
        # frame_options["extraction"] (True, an extraction.ExtractionOptions or an extraction.Extraction; CLI: --spectra /
        # --spectra-only): the device extracts every exposure's column spectra behind its reads; run_observation keeps
        # them in `spectra_result` and writes them to `spectra_out` (an .npz path) when that is set.  `spectra_only`:
        # the reads are neither copied from the device nor written.  frame_options["crrej"] (True or an
        # extraction.CosmicRejection; CLI: --reject-cosmics) rejects cosmic rays in that extraction:
        # `spectra_result["rejected"]` and the .npz's n_rejected then hold each exposure's flag counts.
        # frame_options["channels"] (an extraction.Channels; CLI: --channels LO:HI:N) bins that extraction into
        # flat-fielded wavelength channels: `spectra_result["channels"]` [n, R + 1, C] and the .npz's channels.
        # frame_options["variance"] (True or an extraction.Variances; CLI: --variances [RN]) delivers variances with
        # it: `spectra_result["spectra_var"]` / ["sky_var"] / ["channels_var"] and the .npz's keys of those names.
        # frame_options["optimal"] (True or an extraction.Optimal; CLI: --optimal [H]) adds the optimal extraction on
        # top of those variances: `spectra_result["optimal"]` / ["optimal_var"] and the .npz's keys of those names.
        # frame_options["expected"] ("counts" or "mean"; CLI: --expected): the noise-free expected image of every exposure
        # (wayne_amd/expected.py), on the Exposure and as NNNN_exp.fits beside the raw file.
        # frame_options["ramp_fit"] (True or a rampfit.RampFit; CLI: --rate-images): the ramp fit of every exposure
        # (wayne_amd/rampfit.py), on the Exposure and as NNNN_rate.fits beside the raw file.
        # frame_options["ima"] (True, "rate", "counts" or an ima.Ima; CLI: --ima): the calibrated reads of every exposure
        # (wayne_amd/ima.py), on the Exposure and as NNNN_ima.fits beside the raw file.
        # frame_options["device_fits"] (True; CLI: --device-fits): the device forms the data sections of the _raw files and
        # run_observation writes every file straight from its slot's pinned mirror (fits_delivery) -- the same files,
        # without the host's pass over the samples.  The direct image stays on the host path; not with `spectra_only`.
        self.frame_options = {"out_dtype": np.float32}
        self._fits_active = False    # run_observation's main loop is delivering FITS words (see _generate_exposure)
        self.spectra_out = None
        self.spectra_only = False
        # N > 0 (CLI: --optimal-profile N; needs frame_options["optimal"]): run_observation first forms the visit's
        # profiles from the first N exposures of each group (_build_optimal_profiles) and extracts every exposure with
        # its group's; `optimal_profiles` {extraction.profile_key: Profile} is what it formed, and the .npz also holds
        # optimal_profile_exposures.
        self.optimal_profile_exposures = 0
        self.optimal_profiles = None
        self.spectra_result = None
        self.contaminants = []       # field stars on every exposure (setup_contaminants)
        self.charge_traps = None     # per-pixel charge trapping (setup_charge_traps)
        self.ipc = None              # inter-pixel capacitance (setup_ipc)
        self._trap_tables = None
        self.trap_history = "planned"     # "carried": the device carries each pixel's trap state through the visit
        self.trap_initial_state = None    # [S, S, 2] float32 the carried state starts from (None: the model's `initial`)
        self.trap_state = None            # carried mode: the state after the visit's last exposure (run_observation)
        self._trap_plan = None

    # -- setup_* (observation.py:46-291) ----------------------------------------
    def setup_observation(self, x_ref, y_ref, spatial_scan=False, scan_speed=False):
        self.x_ref, self.y_ref = x_ref, y_ref
        self.spatial_scan, self.scan_speed = spatial_scan, scan_speed

    def setup_contaminants(self, contaminants):
        """Field stars whose first-order spectra land on every exposure of the visit: a list of sources.Contaminant
        (sources.from_config builds them from the YAML's `contaminants:` section); [] or None: the target alone."""
        from .sources import MAX_CONTAMINANTS
        contaminants = list(contaminants or [])
        if len(contaminants) > MAX_CONTAMINANTS:
            raise ValueError("at most %d contaminants" % MAX_CONTAMINANTS)
        self.contaminants = contaminants

    def setup_ipc(self, ipc):
        """Inter-pixel capacitance (ipc.InterpixelCapacitance; ipc.InterpixelCapacitance.from_config builds it from the
        YAML's `interpixel_capacitance:` section; True: the default kernel); None: none.  Every exposure's collected
        charge is then coupled into the neighbouring pixels on the device, in front of the ramp kernel, and the files
        carry IPC = T, IPCUNIT and the nine IPCWij cards.  The direct image is not coupled.  Stateless: it goes with
        sharding, --resume and every other option."""
        from .ipc import as_ipc
        self.ipc = as_ipc(ipc)

    def setup_charge_traps(self, traps, history=None, initial_state=None):
        """Per-pixel charge trapping, the ramp effect (traps.ChargeTraps; traps.ChargeTraps.from_config builds it from the
        YAML's `charge_traps:` section); None: none.  `history` (None: the model's own setting, `traps.history`):
        "planned" -- exposure i gets its start tables from the visit plan (ChargeTraps.start_tables: the visit's history
        at each pixel's own mean rate), so exposures stay independent; "carried" -- the device carries each pixel's trap
        state from exposure to exposure (ChargeTraps.history_plan; run_observation then runs the visit in order on one
        rank and keeps the final state in `trap_state`).  `initial_state`: carried mode only, a [S, S, 2] float32 array
        (bordered frame; [..., 0] slow, [..., 1] fast) the visit starts from in place of the model's `initial` --
        persistence from an earlier visit, or the `trap_state` saved from one."""
        from .traps import ChargeTraps, HISTORIES
        if traps is not None and not isinstance(traps, ChargeTraps):
            raise TypeError("setup_charge_traps: expected traps.ChargeTraps or None")
        if history is None:
            history = traps.history if traps is not None else "planned"
        if history not in HISTORIES:
            raise ValueError("setup_charge_traps: history must be planned or carried, got %r" % (history,))
        if initial_state is not None:
            if traps is None or history != "carried":
                raise ValueError("setup_charge_traps: initial_state needs history='carried'")
            initial_state = np.ascontiguousarray(initial_state, dtype=np.float32)
            if initial_state.ndim != 3 or initial_state.shape[0] != initial_state.shape[1] or initial_state.shape[2] != 2:
                raise ValueError("setup_charge_traps: initial_state has shape (S, S, 2), got %s" % (initial_state.shape,))
        self.charge_traps = traps.with_history(history) if traps is not None else None     # (its cards name the mode)
        self.trap_history = history if traps is not None else "planned"
        self.trap_initial_state = initial_state
        self.trap_state = None
        self._trap_tables = None
        self._trap_plan = None

    @property
    def traps_carried(self):
        return self.charge_traps is not None and self.trap_history == "carried"

    def exposure_traps(self, index):
        """Exposure `index`'s charge traps (traps.ExposureTraps; traps.CarriedTraps in carried mode), or None without
        them."""
        if self.charge_traps is None:
            return None
        if self.traps_carried:
            if self._trap_plan is None:
                exptime = self.detector.exptime(self.NSAMP, self.SUBARRAY, self.SAMPSEQ)
                self._trap_plan = self.charge_traps.history_plan(self.visit_plan, exptime, staring=not self.spatial_scan)
            return self.charge_traps.carried(self._trap_plan, index)
        from .traps import ExposureTraps
        if self._trap_tables is None:
            exptime = self.detector.exptime(self.NSAMP, self.SUBARRAY, self.SAMPSEQ)
            self._trap_tables = self.charge_traps.start_tables(self.visit_plan, exptime, staring=not self.spatial_scan)
        return ExposureTraps(self.charge_traps, self._trap_tables[index])

    def setup_simulator(self, sample_rate=False, clip_values_det_limits=True, threads=2):
        self.sample_rate = sample_rate
        self.clip_values_det_limits = clip_values_det_limits
        self.threads = threads

    def setup_target(self, planet, wavelengths, planet_spectrum, stellar_flux, transittime=None, ldcoeffs=None,
                     period=None, rp=None, sma=None, inclination=None, eccentricity=None, periastron=None,
                     stellar_radius=None, ld_table=None, spots=None):
        """`ld_table` (lightcurve.LimbDarkening): limb darkening per wavelength bin -- the light curves then use
        `ld_table.on_grid(wavelengths)`; `ldcoeffs` stays required: the fallback and the header's LD1 .. LD4.
        `spots` (spots.StarSpots): a spotted star (set_spots)."""
        self.wl = np.asarray(wavelengths, dtype=float)
        self.stellar_flux = np.asarray(stellar_flux, dtype=float)
        self.planet_spectrum = None if planet_spectrum is None else np.asarray(planet_spectrum, dtype=float)
        assert len(self.wl) == len(self.stellar_flux)
        if not isinstance(planet, Planet):
            planet = Planet(name=str(planet))
        self.planet = planet
        if planet_spectrum is not None:
            assert len(self.wl) == len(self.planet_spectrum)
            self.transmission_spectroscopy = True
            for attr, val in (("P", period), ("a", sma), ("i", inclination), ("Rs", stellar_radius),
                              ("transittime", transittime)):
                if val:
                    setattr(planet, attr, val)
            if eccentricity or eccentricity == 0:
                planet.e = eccentricity
            if periastron or periastron == 0:
                planet.periastron = periastron
            if rp:
                planet.rp_over_rs = rp
            if not ldcoeffs:
                raise ValueError("ldcoeffs are required (the reference looks them up with pylightcurve.clablimb, "
                                 "tools.py:220-230, which is not available)")
            self.ldcoeffs = list(ldcoeffs)
            planet.ldcoeffs = self.ldcoeffs          # written into the FITS header (exposure.py:396-402)
            if ld_table is not None and not isinstance(ld_table, lightcurve.LimbDarkening):
                raise TypeError("setup_target: ld_table must be a lightcurve.LimbDarkening or None")
            self.ld_table = ld_table
            self._ld_on_grid = None if ld_table is None else ld_table.on_grid(self.wl)
            planet.ld_table = ld_table               # its cards too, only when there is one
        else:
            if ld_table is not None:
                raise ValueError("setup_target: ld_table needs a planet spectrum (there is no transit without one)")
            self.ld_table = self._ld_on_grid = None
            self.transmission_spectroscopy = False
        self.set_spots(spots)

    def set_spots(self, spots):
        """The star's spots (spots.StarSpots; None: a clean star), after setup_target: the light curves of every path
        (device_depths, generate_lightcurves) are those of the spotted star, and the files carry the SPOTS cards.
        ValueError without a planet spectrum, or when the spotted disc flux is not positive in some bin."""
        from . import spots as _spots
        if spots is None:
            self.spots = self._spot_contrast = None
            if getattr(self, "planet", None) is not None:
                self.planet.spot_cards = None
            return
        if not isinstance(spots, _spots.StarSpots):
            raise TypeError("set_spots: spots must be a spots.StarSpots or None")
        if not self.transmission_spectroscopy:
            raise ValueError("set_spots: spots need a planet spectrum (there is no transit without one)")
        spots.check_flux(self._limb_darkening(), self.wl)
        self.spots = spots
        self._spot_contrast = spots.on_grid(self.wl)
        self.planet.spot_cards = spots.cards(self.wl)       # only when there are spots

    def planet_position_at_phase(self, phase):
        """(X, Y) of the planet's centre on the sky, in stellar radii, `phase` periods from mid-transit."""
        period, sma, e, inc, peri, _ = self._orbit_args()
        X, Y, _ = lightcurve.planet_position(period, sma, e, inc, peri, 0.0, np.array([float(phase) * period]))
        return float(X[0]), float(Y[0])

    def _spot_geometry(self, X, Y, white=False):
        """spots.SpotGeometry of the track X, Y (None: a clean star); `white`: one depth for the whole band, the band
        mean of every spot's contrast."""
        if getattr(self, "spots", None) is None:
            return None
        from . import spots as _spots
        contrast = self._spot_contrast.mean(axis=1, keepdims=True) if white else self._spot_contrast
        return _spots.SpotGeometry(X, Y, self.spots.cx, self.spots.cy, self.spots.radius, contrast)

    def setup_detector(self, detector, NSAMP, SAMPSEQ, SUBARRAY):
        self.detector, self.NSAMP, self.SAMPSEQ, self.SUBARRAY = detector, NSAMP, SAMPSEQ, SUBARRAY

    def setup_grism(self, grism):
        self.grism = grism
        if self.calibration is None:
            self.calibration = grism.calibration

    def setup_visit(self, start_JD, num_orbits, exp_start_times=False):
        self.start_JD, self.num_orbits = start_JD, num_orbits
        if exp_start_times is not False and exp_start_times is not None and len(np.atleast_1d(exp_start_times)):
            self.exp_start_times = np.asarray(exp_start_times, dtype=float)
            self.visit_plan = {"exp_start_times": self.exp_start_times,
                               "orbit_start_index": tools.detect_orbits(self.exp_start_times)}
        else:
            self.visit_plan = VisitPlanner(self.detector, self.NSAMP, self.SAMPSEQ, self.SUBARRAY, self.num_orbits,
                                           exp_overhead=3.0)            # observation.py:229-233
            self.exp_start_times = self.visit_plan["exp_times"] / (24. * 60.) + self.start_JD
            self.visit_plan["exp_start_times"] = self.exp_start_times
        self._trap_tables = None
        self._trap_plan = None

    def setup_reductions(self, add_dark=True, add_flat=True, add_gain_variations=True, add_non_linear=True,
                         add_initial_bias=True):
        self.add_dark, self.add_flat = add_dark, add_flat
        self.add_gain_variations, self.add_non_linear = add_gain_variations, add_non_linear
        self.add_initial_bias = add_initial_bias

    def setup_trends(self, ssv_gen, x_shifts=0, x_jitter=0.0000001, y_shifts=0, y_jitter=0.0000001):
        self.ssv_gen = ssv_gen
        self.x_shifts, self.x_jitter, self.y_shifts, self.y_jitter = x_shifts, x_jitter, y_shifts, y_jitter

    def setup_noise_sources(self, sky_background=1.0, cosmic_rate=11., add_read_noise=True, add_stellar_noise=True):
        self.sky_background, self.cosmic_rate = sky_background, cosmic_rate
        self.add_read_noise, self.add_stellar_noise = add_read_noise, add_stellar_noise

    def setup_gaussian_noise(self, noise_mean=False, noise_std=False):
        self.noise_mean, self.noise_std = noise_mean, noise_std

    def setup_visit_trend(self, visit_trend_coeffs):
        self._visit_trend = visit_trends.HookAndLongTermRamp(self.visit_plan, visit_trend_coeffs)

    # -- light curves ---------------------------------------------------------------
    def _orbit_args(self):
        p = self.planet
        W = p.periastron
        if W is None or (isinstance(W, float) and np.isnan(W)):
            W = 0.0
        return (float(p.P), float(p.sma_over_rs), float(p.e or 0.0), float(p.i), float(W), float(p.transittime))

    def generate_lightcurves(self, time_array, depth=False):
        """Normalised flux, shape (len(time_array), n_depths) (observation.py:293-357).
        The reference converts JD to HJD for the target's catalogue coordinates (observation.py:340,
        tools.py:220-271); here that happens when the planet carries ra_deg / dec_deg (there is no
        catalogue to look them up in), else times are used as given."""
        time_array = self._to_hjd(time_array)
        spectrum = np.array([depth]) if depth else self.planet_spectrum
        rp_white = self.planet.rp_over_rs or float(np.sqrt(np.mean(self.planet_spectrum)))
        z_tr, hidden, X, Y = lightcurve.depth_inputs_track(*(self._orbit_args() + (time_array, rp_white)))
        return 1.0 - lightcurve.planet_depths(self._limb_darkening(white=bool(depth)), spectrum, z_tr, hidden,
                                              spots=self._spot_geometry(X, Y, white=bool(depth)))

    def _limb_darkening(self, white=False):
        """What the light curves take as `ld`: the four coefficients, or with a table its coefficients on the visit's
        wavelength grid [W, 4] (`white`: one depth for the whole band -- the table's mean profile over the grid, which is
        the mean of its coefficients, I being linear in them)."""
        table = getattr(self, "_ld_on_grid", None)
        if table is None:
            return self.ldcoeffs
        return table.mean(axis=0, keepdims=True) if white else table

    def device_depths(self, time_array):
        """The same per-sub-sample depths, as the recipe the GPU evaluates."""
        rp_white = self.planet.rp_over_rs or float(np.sqrt(np.mean(self.planet_spectrum)))
        z_tr, hidden, X, Y = lightcurve.depth_inputs_track(*(self._orbit_args() + (self._to_hjd(time_array), rp_white)))
        return lightcurve.DeviceDepths(z_tr, hidden, self.planet_spectrum, self._limb_darkening(),
                                       spots=self._spot_geometry(X, Y))

    def _to_hjd(self, time_array):
        p = self.planet
        if getattr(p, "ra_deg", None) is None or getattr(p, "dec_deg", None) is None:
            return time_array
        return tools.jd_to_hjd(time_array, p.ra_deg, p.dec_deg)

    def show_lightcurve(self):
        """White light curve of the planned visit -> (times, model); the reference also plots it."""
        t = self.exp_start_times
        if self.transmission_spectroscopy:
            depth = self.planet.rp_over_rs ** 2 if self.planet.rp_over_rs else float(np.mean(self.planet_spectrum))
            lc_model = self.generate_lightcurves(t, depth).T[0]
        else:
            lc_model = np.ones_like(t)
        if self._visit_trend:
            lc_model = np.asarray(self._visit_trend.scale_factors)[:len(lc_model)] * lc_model
        return t, lc_model

    # -- running ----------------------------------------------------------------------
    @staticmethod
    def _try_index(value, index):
        try:
            return value[index]
        except (TypeError, IndexError):
            return value

    def exposure_file_is_whole(self, number):
        """Is `NNNN_raw.fits` of exposure `number` (1-based) in the output directory, complete, and THIS visit's file?
        Files are written under a temporary name and renamed when finished (fitsio.write_pieces), so a file under its
        final name is whole unless something else truncated it: checked anyway -- the HDU structure is walked header by
        header (1 + 5 NSAMP HDUs ending exactly at the end of the file, SCI images of the mode's size and of the sample
        type this visit writes) and the primary
        header must carry this exposure's start time and mode."""
        path = os.path.join(self.outdir, "{:04d}_raw.fits".format(number))
        if not os.path.isfile(path):
            return False
        from . import fitsio
        hdus = fitsio.scan(path)
        if hdus is None or len(hdus) != 1 + 5 * self.NSAMP:
            return False
        p0 = hdus[0][0]
        S = self.detector.frame_size(self.SUBARRAY) if hasattr(self.detector, "frame_size") else (
            1024 if self.SUBARRAY == 1024 else self.SUBARRAY + 10)
        try:
            same = (int(p0["NSAMP"]) == self.NSAMP and str(p0["SAMP_SEQ"]).strip() == self.SAMPSEQ and
                    abs(float(p0["EXPSTART"]) - (float(self.exp_start_times[number - 1]) - 2400000.5)) < 1e-7)
        except (KeyError, TypeError, ValueError):
            return False
        if not (same and self._contaminant_cards_match(p0) and self._trap_cards_match(p0) and self._ld_cards_match(p0) and
                self._ipc_cards_match(p0) and self._spot_cards_match(p0)):
            return False
        # the visit's sample type too: uint16 reads make BITPIX 16 images, float reads float64 ones -- a file of the
        # other kind is regenerated, whichever way the visit was switched
        elem = 2 if np.dtype(self.frame_options.get("out_dtype", np.float32)) == np.uint16 else 8
        return all(size == S * S * elem for (h, size) in hdus[1::5])

    def _contaminant_cards_match(self, p0):
        """The file's NCONTAM / CONTDXn / CONTDYn / CONTFRn cards are this visit's contaminants (absent: none), so that
        --resume after a contaminant was added or changed regenerates the files instead of mixing two fields."""
        from .exposure import contaminant_cards
        want = {k: v for (k, v, _) in contaminant_cards(self.contaminants)} if self.contaminants else {}
        try:
            if "NCONTAM" not in p0:
                return not want
            if not want or int(p0["NCONTAM"]) != want["NCONTAM"]:
                return False
            return all(abs(float(p0[k]) - float(v)) <= 1e-9 * max(1.0, abs(float(v))) for k, v in want.items())
        except (KeyError, TypeError, ValueError):
            return False

    def _ld_cards_match(self, p0):
        """The file's LDTABLE / LDLAW / LDNODES / LDWLLO / LDWLHI / LDHASH cards are this visit's limb-darkening table
        (absent: none), so that --resume after a table was added, removed or changed regenerates the files."""
        table = getattr(self, "ld_table", None)
        want = {k: v for (k, v, _) in table.cards()} if table is not None else {}
        try:
            if "LDTABLE" not in p0:
                return not want
            if not want or p0["LDTABLE"] is not True:
                return False
            return (str(p0["LDHASH"]).strip() == want["LDHASH"] and str(p0["LDLAW"]).strip() == want["LDLAW"] and
                    int(p0["LDNODES"]) == want["LDNODES"])
        except (KeyError, TypeError, ValueError):
            return False

    def _spot_cards_match(self, p0):
        """The file's SPOTS / NSPOTS / SPTHASH cards are this visit's star spots (absent: none), so that --resume after a
        spot was added, removed or changed regenerates the files."""
        cards = getattr(getattr(self, "planet", None), "spot_cards", None)
        want = {k: v for (k, v, _) in cards} if cards else {}
        try:
            if "SPOTS" not in p0:
                return not want
            if not want or p0["SPOTS"] is not True:
                return False
            return str(p0["SPTHASH"]).strip() == want["SPTHASH"] and int(p0["NSPOTS"]) == want["NSPOTS"]
        except (KeyError, TypeError, ValueError):
            return False

    def _ipc_cards_match(self, p0):
        """The file's IPC / IPCUNIT / IPCWij cards are this visit's inter-pixel capacitance (absent: none), so that
        --resume after the kernel was added, removed or changed regenerates the files."""
        want = {k: v for (k, v, _) in self.ipc.cards()} if self.ipc is not None else {}
        try:
            if "IPC" not in p0:
                return not want
            if not want or p0["IPC"] is not True:
                return False
            return all(int(p0[k]) == int(v) for k, v in want.items() if k != "IPC")
        except (KeyError, TypeError, ValueError):
            return False

    def _trap_cards_match(self, p0):
        """The file's CTRAPS and CT* cards are this visit's charge traps (absent: none), so that --resume after the model
        or its start tables' grid was switched on, off or changed regenerates the files."""
        want = {k: v for (k, v, _) in self.charge_traps.cards()} if self.charge_traps is not None else {}
        try:
            if "CTRAPS" not in p0:
                return not want
            if not want or p0["CTRAPS"] is not True:
                return False
            return all(abs(float(p0[k]) - float(v)) <= 1e-9 * max(1.0, abs(float(v)))
                       for k, v in want.items() if k != "CTRAPS")
        except (KeyError, TypeError, ValueError):
            return False

    def run_observation(self, rank=0, world=1, write_fits=True, resume=False):
        """Generate the direct image and every exposure (observation.py:388-413); with
        world > 1 only the exposures i = rank, rank + world, ... (round-robin sharding).
        `resume`: an exposure whose file is already in the output directory, whole and this visit's
        (exposure_file_is_whole), is not generated again -- what is left of a visit after a rank died is then only the
        files that are missing.  Every exposure's random streams are keyed by the visit seed and its own index, so the
        files of a resumed visit are those of an uninterrupted one (the reference, whose exposures share one global
        numpy stream, has no such restart: it deletes and rewrites, exposure.py:211-213).
        With frame_options["extraction"] every exposure's spectra are delivered too (see __init__): `spectra_result`
        holds them and `spectra_out` names the .npz they are written to -- with world > 1 each rank writes its own,
        `.rankNN` before the extension.  Not together with `resume` (a skipped exposure has no spectra)."""
        extraction = self.frame_options.get("extraction")
        if extraction is None and (self.spectra_only or self.spectra_out):
            raise ValueError("spectra_out / spectra_only need frame_options['extraction']")
        if extraction is not None and resume:
            raise ValueError("spectra are not delivered by a resumed visit: the exposures it skips have none")
        device_fits = bool(self.frame_options.get("device_fits", False))
        if device_fits and self.spectra_only:
            raise ValueError("device_fits forms the data sections of the raw files; spectra_only writes none")
        # frame_options["expected"] ("counts" / "mean"; CLI: --expected): every exposure's noise-free expected image is
        # rendered beside it (wayne_amd/expected.py) -- the Exposure carries it and NNNN_exp.fits is written beside the raw file
        from . import expected as _expected
        expected = self.frame_options.get("expected")
        _expected.refuse_combinations(expected, resume=resume, device_fits=device_fits, spectra=extraction is not None,
                                      spectra_only=self.spectra_only)
        # frame_options["ramp_fit"] (True or a rampfit.RampFit; CLI: --rate-images): every exposure's ramps are fitted on the
        # device (wayne_amd/rampfit.py) -- the Exposure carries the planes and NNNN_rate.fits is written beside the raw file
        from . import rampfit as _rampfit
        ramp_fit = _rampfit.as_ramp_fit(self.frame_options.get("ramp_fit"))
        _rampfit.refuse_combinations(ramp_fit, resume=resume, device_fits=device_fits, spectra_only=self.spectra_only)
        # frame_options["ima"] (True, "rate", "counts" or an ima.Ima; CLI: --ima): every exposure's calibrated reads are formed
        # on the device (wayne_amd/ima.py) -- the Exposure carries the payload and NNNN_ima.fits is written beside the raw file
        from . import ima as _ima
        ima = _ima.as_ima(self.frame_options.get("ima"))
        _ima.refuse_combinations(ima, resume=resume, device_fits=device_fits, spectra_only=self.spectra_only)
        if self.traps_carried:
            # every exposure starts from the state its predecessor left on ONE device: the visit runs whole and in order
            if world > 1:
                raise ValueError("charge_traps history: carried -- the visit cannot be sharded (world > 1)")
            if resume:
                raise ValueError("charge_traps history: carried -- resume=True would skip exposures the state depends on")
            if self.optimal_profile_exposures:
                raise ValueError("charge_traps history: carried -- optimal_profile_exposures runs exposures in a first "
                                 "pass, which would advance the trap state")
        if self.spectra_only:
            write_fits_raw = False
        else:
            write_fits_raw = write_fits
        if write_fits and self.outdir and not os.path.exists(self.outdir):
            os.makedirs(self.outdir)
        frames = {}
        if write_fits and self.outdir:
            # a crash leaves at most half-written temporary files behind: this rank's are removed (never a final name)
            from . import fitsio
            for i in [-1] + list(range(rank, len(self.exp_start_times), world)):
                if i == -1 and rank != 0:
                    continue
                name = "0000_flt.fits" if i == -1 else "{:04d}_raw.fits".format(i + 1)
                part = os.path.join(self.outdir, name + fitsio.PART_SUFFIX)
                if os.path.exists(part):
                    os.remove(part)
        if rank == 0 and not (resume and write_fits and os.path.isfile(os.path.join(self.outdir, "0000_flt.fits"))
                              and self._fits_is_whole(os.path.join(self.outdir, "0000_flt.fits"))):
            frames[0] = self._generate_direct_image(write_fits)
        mine = list(range(rank, len(self.exp_start_times), world))
        self.skipped = []
        if resume and write_fits:
            self.skipped = [i for i in mine if self.exposure_file_is_whole(i + 1)]
            done = set(self.skipped)
            mine = [i for i in mine if i not in done]
        # The context is created HERE, on the thread that will use it (upload / run / wait): the producer's prepare()
        # then finds the engine in the cache instead of building the context, uploading grism and calibration, on its
        # own thread.
        from . import engine as _engine
        opts = dict(self.frame_options)
        eng = _engine.get_engine(self.device, self.grism, self.detector, self.calibration, self.NSAMP, self.SAMPSEQ,
                                 self.SUBARRAY, opts.get("add_initial_bias", self.add_initial_bias),
                                 g102_flat_quirk=bool(opts.get("reference_quirks", False)))
        # files are written by background threads while the GPU works on the next exposures
        from .exposure import FitsWriterPool
        from .pipeline import run_pipelined
        pool = FitsWriterPool() if write_fits_raw else None
        fits = device_fits and pool is not None       # (no raw files: nothing to form on the device)
        got_spectra = []            # (index, spectra, sky, plan, x_ref, y_ref, n_rejected or None, channels or None) of every exposure, in delivery order; then its variances or None, then its (optimal, optimal_var) or None

        def prepare(i):
            gen = self._generate_exposure(self.exp_start_times[i], i + 1, write_fits=False, prepare_only=True)
            return gen._prepared[1], gen

        def finish(i, gen, reads):
            frame = None
            payload = None
            if fits:
                # the file's data sections instead of the reads, which stay on the device
                if extraction is not None:
                    payload, reads = reads[0], (None,) + tuple(reads[1:])
                else:
                    payload, reads = reads, None
            if extraction is not None:
                reads, spectra, sky = reads
                spectra, sky = np.array(spectra), np.array(sky)           # (copies: the pinned buffer is reused)
                got_spectra.append((i, spectra, sky, gen.extraction_plan, gen.exp_info["x_ref"], gen.exp_info["y_ref"],
                                    ctx.rejected, ctx.channels, ctx.variances, ctx.optimal, ctx.channels_opt))
                frame = gen._fill_spectra(spectra, sky, ctx.rejected, ctx.channels, ctx.variances, ctx.optimal,
                                          ctx.profile_planes, ctx.channels_opt)
            if reads is not None:
                frame = gen._fill_exposure(np.array(reads), gen._prepared[2])     # (a copy: the pinned buffer is reused)
            if expected and frame is not None:
                frame.expected = ctx.expected
                if pool is not None:
                    _expected.write_fits(os.path.join(self.outdir, "{:04d}_exp.fits".format(i + 1)), frame, ctx.expected, expected)
            if ramp_fit is not None and frame is not None:
                _rampfit.fill_exposure(frame, ctx.ramp_fit, gen._read_dt)
                if pool is not None:
                    _rampfit.write_fits(os.path.join(self.outdir, "{:04d}_rate.fits".format(i + 1)), frame, ramp_fit)
            if ima is not None and frame is not None:
                frame.ima = ctx.ima
                if pool is not None:
                    _ima.write_fits(os.path.join(self.outdir, "{:04d}_ima.fits".format(i + 1)), frame)
            if payload is not None:
                # (views of the pinned mirror, no copy: the slot is not uploaded again until the writer has released it)
                frame = gen._fill_stored(payload, ctx.layout, gen._prepared[2])
                pool.submit(frame, self.outdir, "{:04d}_raw.fits".format(i + 1), done=ctx.lease())
                frames[i + 1] = None
            elif pool is not None:
                pool.submit(frame, self.outdir, "{:04d}_raw.fits".format(i + 1))
                frames[i + 1] = None          # on disk; do not keep 64 MB per exposure alive
            else:
                frames[i + 1] = frame

        if extraction is not None and self.optimal_profile_exposures:
            self._build_optimal_profiles(mine, eng.ctx)
        if self.traps_carried:
            if self.trap_initial_state is not None:
                eng.ctx.trap_state_upload(self.trap_initial_state)
            else:
                eng.ctx.trap_state_reset(self.charge_traps.array("initial"))
            self.trap_state = None
        try:
            # up to 3 exposures in flight on 4 context slots in rotation (even / odd slots run on different HIP streams)
            ctx = eng.ctx
            n_slots = 4
            if extraction is not None:
                from .extraction import Delivery
                ctx = Delivery(eng.ctx, reads=not self.spectra_only and not fits)
            if fits:
                # ... on more slots than that: a slot's pinned mirror belongs to its file until a writer has it out
                from .fits_delivery import FitsDelivery, slots_for
                ctx = FitsDelivery(eng.ctx, extraction=ctx if extraction is not None else None)
                n_slots = slots_for(4, pool.n_threads)
                self._fits_active = True
            if expected:
                ctx = _expected.ExpectedDelivery(eng.ctx, ctx)
            if ramp_fit is not None:
                ctx = _rampfit.RampFitDelivery(eng.ctx, ctx)
            if ima is not None:
                ctx = _ima.ImaDelivery(eng.ctx, ctx)
            run_pipelined(ctx, mine, prepare, finish, depth=3, n_slots=n_slots)
        finally:
            self._fits_active = False
            if pool is not None:
                pool.close()
        if self.traps_carried:
            self.trap_state = eng.ctx.trap_state_download()
        if extraction is not None:
            self._keep_spectra(got_spectra, rank, world)
        return frames

    def _build_optimal_profiles(self, mine, ctx):
        """The first pass of `optimal_profile_exposures` = N: the first N exposures of each group among `mine` -- a group
        is what extraction.profile_key tells apart, window heights and scan direction, so a visit whose windows change
        height as the star drifts over a row boundary has several -- are synthesised with their profile planes delivered
        (the reads never leave the device), each group's planes are added up and normalised, and
        frame_options["optimal"] then carries {key: Profile}: every exposure of the visit proper is extracted with its
        group's.  Every exposure's host half runs once more for it (its plan tells its group).  With several ranks each
        forms its profiles from its own share."""
        from . import extraction as _extraction
        from .pipeline import run_pipelined
        optimal = _extraction.Optimal.coerce(self.frame_options.get("optimal"))
        if optimal is None:
            raise ValueError("optimal_profile_exposures needs frame_options['optimal']")
        n = int(self.optimal_profile_exposures)
        kept = dict(self.frame_options)
        seen, first = {}, []
        self.frame_options = dict(kept, optimal=optimal.with_profile(None))
        try:
            for i in mine:
                gen = self._generate_exposure(self.exp_start_times[i], i + 1, write_fits=False, prepare_only=True)
                key = gen.profile_key
                if seen.get(key, 0) < n:
                    seen[key] = seen.get(key, 0) + 1
                    first.append((i, key))
            keys = dict(first)
            sums = {}
            # (the optimal channels of these exposures would be thrown away: off)
            self.frame_options = dict(kept, optimal=optimal.with_profile(None, deliver_profile=True, channels=False))
            delivery = _extraction.Delivery(ctx, reads=False)

            def prepare(i):
                gen = self._generate_exposure(self.exp_start_times[i], i + 1, write_fits=False, prepare_only=True)
                return gen._prepared[1], gen

            def finish(i, gen, got):
                sums.setdefault(keys[i], _extraction.ProfileSum()).add(gen.extraction_plan, delivery.profile_planes)

            run_pipelined(delivery, [i for i, _ in first], prepare, finish, depth=3, n_slots=4)
        finally:
            self.frame_options = kept
        self.optimal_profiles = {key: acc.profile() for key, acc in sums.items()}
        self.frame_options = dict(kept, optimal=optimal.with_profile(self.optimal_profiles, optimal.deliver_profile))

    def _keep_spectra(self, got, rank, world):
        """What the exposures' extraction delivered -> `spectra_result` (the arrays of extraction.save_npz), written to
        `spectra_out` when that is set."""
        from . import extraction as _extraction
        got = sorted(got, key=lambda g: g[0])
        idx = [g[0] for g in got]
        self.spectra_result = dict(
            spectra=np.array([g[1] for g in got]), sky=np.array([g[2] for g in got]), exposure_index=np.array(idx, dtype=int),
            plans=[g[3] for g in got], x_ref=np.array([g[4] for g in got], dtype=float),
            y_ref=np.array([g[5] for g in got], dtype=float),
            read_times=np.asarray(self.detector.get_read_times(self.NSAMP, self.SUBARRAY, self.SAMPSEQ), dtype=float),
            exp_start=np.asarray(self.exp_start_times, dtype=float)[idx] if idx else np.zeros(0))
        if got and all(g[6] is not None for g in got):        # extracted with cosmic-ray rejection: the flag counts
            self.spectra_result["rejected"] = np.array([g[6] for g in got], dtype=np.uint32)
        if got and all(g[7] is not None for g in got):        # binned into wavelength channels
            self.spectra_result["channels"] = np.array([g[7] for g in got], dtype=np.float64)
        if got and all(g[8] is not None for g in got):        # extracted with variances
            self.spectra_result["spectra_var"] = np.array([g[8][0] for g in got], dtype=np.float64)
            self.spectra_result["sky_var"] = np.array([g[8][1] for g in got], dtype=np.float64)
            if all(g[8][2] is not None for g in got):
                self.spectra_result["channels_var"] = np.array([g[8][2] for g in got], dtype=np.float64)
        if got and all(g[9] is not None for g in got):        # extracted optimally too
            self.spectra_result["optimal"] = np.array([g[9][0] for g in got], dtype=np.float64)
            self.spectra_result["optimal_var"] = np.array([g[9][1] for g in got], dtype=np.float64)
        if got and all(g[10] is not None for g in got):       # the optimal channels
            self.spectra_result["channels_opt"] = np.array([g[10][0] for g in got], dtype=np.float64)
            self.spectra_result["channels_opt_var"] = np.array([g[10][1] for g in got], dtype=np.float64)
        if not self.spectra_out:
            return None
        path = self.spectra_out
        if world > 1:
            root, ext = os.path.splitext(path)
            path = "%s.rank%02d%s" % (root, rank, ext)
        r = self.spectra_result
        with open(path, "wb") as f:
            _extraction.save_npz(f, r["spectra"], r["sky"], r["exposure_index"], r["plans"], r["x_ref"], r["y_ref"],
                                 r["read_times"], r["exp_start"], rejected=r.get("rejected"), channels=r.get("channels"),
                                 variances=(r["spectra_var"], r["sky_var"], r.get("channels_var")) if "spectra_var" in r else None,
                                 optimal=(r["optimal"], r["optimal_var"]) if "optimal" in r else None,
                                 optimal_profile_exposures=self.optimal_profile_exposures if "optimal" in r else None,
                                 channels_opt=(r["channels_opt"], r["channels_opt_var"]) if "channels_opt" in r else None)
        return path

    @staticmethod
    def _fits_is_whole(path):
        from . import fitsio
        return fitsio.scan(path) is not None

    def _generate_exposure(self, expstart, number, write_fits=True, prepare_only=False):
        """observation.py:415-504.  With `prepare_only` only the exposure's host half runs and the ExposureGenerator is
        returned (ExposureGenerator.prepare): run_observation's loop does the rest on the context's thread."""
        index_number = number - 1
        filename = "{:04d}_raw.fits".format(number)
        exp_gen = ExposureGenerator(self.detector, self.grism, self.NSAMP, self.SAMPSEQ, self.SUBARRAY, self.planet,
                                    filename, expstart, calibration=self.calibration, device=self.device,
                                    seed=self.seed, exposure_index=index_number)
        sample_rate = self.sample_rate if self.spatial_scan else 365.25 * 86400. * 1000.
        _, sample_mid_points, sample_durations, read_index = exp_gen._gen_scanning_sample_times(sample_rate)
        time_array = expstart + sample_mid_points / (86400. * 1000.)
        planet_depths = self.device_depths(time_array) if self.transmission_spectroscopy else None
        x_ref = self._try_index(self.x_ref, index_number) + self.x_shifts * index_number
        y_ref = self._try_index(self.y_ref, index_number) + self.y_shifts * index_number
        sky_background = self._try_index(self.sky_background, index_number)
        scale_factor = self._visit_trend.get_scale_factor(index_number) if self._visit_trend else None
        common = dict(noise_mean=self.noise_mean, noise_std=self.noise_std, add_flat=self.add_flat,
                      add_dark=self.add_dark, scale_factor=scale_factor, sky_background=sky_background,
                      cosmic_rate=self.cosmic_rate, add_gain_variations=self.add_gain_variations,
                      add_non_linear=self.add_non_linear, clip_values_det_limits=self.clip_values_det_limits,
                      add_read_noise=self.add_read_noise, add_stellar_noise=self.add_stellar_noise,
                      add_initial_bias=self.add_initial_bias, threads=self.threads)
        common.update(self.frame_options)
        # (device_fits belongs to run_observation's file-writing loop: only its descriptors ask for the FITS words)
        if common.pop("device_fits", False) and prepare_only and self._fits_active:
            common["device_fits"] = True
        if self.contaminants:
            common["contaminants"] = self.contaminants
        if self.charge_traps is not None:
            common["charge_traps"] = self.exposure_traps(index_number)
        if self.ipc is not None:
            common["ipc"] = self.ipc
        if self.spatial_scan:
            args = (x_ref, y_ref, self.x_jitter, self.y_jitter, self.wl, self.stellar_flux, planet_depths,
                    self.scan_speed, sample_rate, sample_mid_points, sample_durations, read_index)
            common["ssv_generator"] = self.ssv_gen
        else:
            args = (x_ref, y_ref, self.x_jitter, self.y_jitter, self.wl, self.stellar_flux, planet_depths,
                    sample_mid_points, sample_durations, read_index)
        if prepare_only:
            return exp_gen.prepare(*args, staring=not self.spatial_scan, **common)
        exp_frame = exp_gen.scanning_frame(*args, **common) if self.spatial_scan else exp_gen.staring_frame(*args, **common)
        if write_fits:
            exp_frame.generate_fits(self.outdir, filename)
        return exp_frame

    def _generate_direct_image(self, write_fits=True):
        """observation.py:516-538."""
        di_start_JD = self.exp_start_times[0] - 1.0 / (24. * 60.)
        gen = ExposureGenerator(self.detector, self.grism, self.NSAMP, self.SAMPSEQ, self.SUBARRAY, self.planet,
                                "0000_flt.fits", di_start_JD, calibration=self.calibration, device=self.device)
        exp = gen.direct_image(self._try_index(self.x_ref, 0), self._try_index(self.y_ref, 0))
        if write_fits:
            exp.generate_fits(self.outdir, "0000_flt.fits")
        return exp
