"""ExposureGenerator: builds one up-the-ramp WFC3-IR exposure.

Same class name, constructor and `scanning_frame` / `staring_frame` argument
lists as the reference (wayne/exposure_generator.py:16-58, 146-192), with
plain floats in fixed units instead of astropy Quantities:

    wl              micron            scan_speed      pixel / second
    sample_rate     millisecond       sample_mid_points / sample_durations   millisecond
    sky_background  counts / second   read times      second

What differs is where the work runs.  The reference loops over sub-samples on
the host (exposure_generator.py:336-394), calling the C thrower and several
full-frame numpy passes per sub-sample; here the host only prepares the small
K-vectors (sample timing, scan positions, jitter, SSV) and one descriptor, and
the whole exposure -- trace, counts, electron thrower, flat, sky, cosmic rays,
gain, dark, non-linearity, clipping, zero read, read noise -- is synthesised
by five HIP kernels through wayne_exposure_synthesize (include/wayne_hip.h).

Random numbers: the reference consumes one global MT19937 stream in exposure
order (run_visit.py:68-77); here every draw is a Philox counter keyed by
(seed, stage, exposure index, sub-sample | read, element), so exposures can be
generated in any order on any GPU with identical results.
"""
import time
import warnings

import numpy as np

from . import _lib, engine as _engine, exposure, lightcurve, tools
from . import traps as _traps
from . import extraction as _extraction
from . import rampfit as _rampfit
from . import ima as _ima
from . import ipc as _ipc
from .trend_generators import scan_speed_varations

MS_PER_YEAR = 365.25 * 86400. * 1000.
_CROP_CACHE = {}      # spectrum grid -> crop indices (build_descriptor)
_TIMES_CACHE = {}     # (read times, sample rate) -> sample starts / mid points / durations / read index


class WFC3SimNoDarkFileWarning(Warning):
    pass


class ExposureGenerator(object):
    def __init__(self, detector, grism, NSAMP, SAMPSEQ, SUBARRAY, planet=None,
                 filename="0001_raw.fits", start_JD=0.0, calibration=None, device=0, seed=0,
                 exposure_index=0):
        """:param calibration: wayne_amd.calibration.CalibrationSet (defaults to grism.calibration)
        :param device: GPU ordinal; :param seed: visit seed; :param exposure_index: extends
        every RNG counter so that exposures of a visit draw independent numbers."""
        self.detector, self.grism, self.planet = detector, grism, planet
        self.NSAMP, self.SAMPSEQ, self.SUBARRAY = NSAMP, SAMPSEQ, SUBARRAY
        self.calibration = calibration if calibration is not None else grism.calibration
        self.device, self.seed, self.exposure_index = device, seed, exposure_index
        self._prepared = None      # (engine, descriptor, start time) of prepare()

        self.exptime = self.detector.exptime(NSAMP, SUBARRAY, SAMPSEQ)             # s
        self.read_times = self.detector.get_read_times(NSAMP, SUBARRAY, SAMPSEQ)   # s

        self.exp_info = {
            "filename": filename, "EXPSTART": start_JD, "EXPEND": start_JD + self.exptime / 86400.,
            "EXPTIME": self.exptime, "SCAN": False, "SCAN_DIR": None, "OBSTYPE": "SPECTROSCOPIC",
            "NSAMP": NSAMP, "SAMPSEQ": SAMPSEQ, "SUBARRAY": SUBARRAY, "samp_rate": 0.0, "sim_time": 0.0,
            "scan_speed_var": False, "noise_mean": False, "noise_std": False, "add_dark": False,
            "add_stellar_noise": False, "seed": seed,
        }

    # -- sample timing (host, K-vectors) ----------------------------------------
    def _gen_scanning_sample_times(self, sample_rate):
        """Sub-sample start / mid / duration (ms) and the index of the last
        sub-sample of each read (exposure_generator.py:531-579): sample at
        `sample_rate` from the previous read up to each read; the last sample
        before a read is cut short so that it ends on the read."""
        key = (tuple(float(t) for t in self.read_times), float(sample_rate))
        hit = _TIMES_CACHE.get(key)
        if hit is None:
            read_times = self.read_times * 1000.
            starts, read_index, i, previous = [], [], -1, 0.
            for read_time in read_times:
                s = np.arange(previous, read_time, sample_rate)
                starts.append(s)
                i += len(s)
                read_index.append(i)
                previous = read_time
            sample_starts = np.concatenate(starts)
            ends = np.roll(sample_starts, -1)
            ends[-1] = read_times[-1]
            sample_durations = ends - sample_starts
            sample_mid_points = sample_starts + (sample_durations / 2)
            if len(_TIMES_CACHE) > 16:
                _TIMES_CACHE.clear()
            hit = _TIMES_CACHE[key] = (sample_starts, sample_mid_points, sample_durations, read_index)
        # (the same numbers for every exposure of a visit; handed out as copies: callers scale the durations)
        return hit[0].copy(), hit[1].copy(), hit[2].copy(), list(hit[3])

    def _gen_sample_yref(self, y_ref, mid_points, scan_speed):
        """y of the star at each sub-sample mid-point; scan_speed in px/ms (:517-529)."""
        return y_ref + (np.asarray(mid_points, dtype=float) * scan_speed)

    # -- exposures ---------------------------------------------------------------
    @staticmethod
    def _staring_as_scan(x_ref, y_ref, x_jitter, y_jitter, wl, stellar_flux, planet_signal,
                         sample_mid_points, sample_durations, read_index, noise_mean, noise_std, add_dark,
                         add_flat, cosmic_rate, sky_background, scale_factor, add_gain_variations,
                         add_non_linear, clip_values_det_limits, add_read_noise, add_stellar_noise,
                         add_initial_bias, progress_bar=None, threads=2, **kw):
        """staring_frame's argument list (the reference's, :146-176) as scanning_frame's -> (args, keywords)."""
        return (x_ref, y_ref, x_jitter, y_jitter, wl, stellar_flux, planet_signal, 0.0, MS_PER_YEAR,
                sample_mid_points, sample_durations, read_index, None, noise_mean, noise_std, add_dark, add_flat,
                cosmic_rate, sky_background, scale_factor, add_gain_variations, add_non_linear,
                clip_values_det_limits, add_read_noise, add_stellar_noise, add_initial_bias, progress_bar,
                threads), kw

    def staring_frame(self, *args, **kw):
        """A staring exposure is a scan at speed 0 sampled once per read (:146-176); arguments: _staring_as_scan."""
        args, kw = self._staring_as_scan(*args, **kw)
        return self.scanning_frame(*args, **kw)

    def scanning_frame(self, x_ref, y_ref, x_jitter, y_jitter, wl, stellar_flux, planet_signal,
                       scan_speed, sample_rate, sample_mid_points=None, sample_durations=None,
                       read_index=None, ssv_generator=None, noise_mean=False, noise_std=False,
                       add_dark=True, add_flat=True, cosmic_rate=None, sky_background=1.0,
                       scale_factor=None, add_gain_variations=True, add_non_linear=True,
                       clip_values_det_limits=True, add_read_noise=True, add_stellar_noise=True,
                       add_initial_bias=True, progress_bar=None, threads=2,
                       rng_mode=_lib.RNG_SPLIT, out_dtype=np.float32, reference_quirks=False,
                       record=None, exact_samplers=False, contaminants=None, charge_traps=None, extraction=None,
                       crrej=None, channels=None, variance=None, optimal=None, expected=None, ramp_fit=None, ima=None, ipc=None):
        """Generate a spatially scanned exposure (exposure_generator.py:178-405).

        Extra keywords (not in the reference): `rng_mode` -- RNG_SPLIT (default:
        Philox-keyed streams, wide PSF component thrown per electron, narrow
        component drawn as one multinomial per bin), RNG_PHILOX (every electron
        thrown), or RNG_REPLAY (the reference's rand_r streams in the thrower,
        with `threads` selecting its OpenMP partition: bit-exact scatter); `out_dtype` -- float32 reads (the
        default HERE and in Observation, VisitRunner, the CLI and bench.py's `value`: ONE arithmetic for every entry
        point -- exact integer electron sums, then a float32 per-read chain; half the bytes to write and to carry
        over PCIe, <= 3 ulp of a float32 from the float64 result, no measurable effect on a recovered transit depth:
        profiles/r06/visit_science.json) or float64 reads (out_dtype=np.float64, CLI --float64-reads: what the
        reference's Exposure.reads hold, exposure.py:47,106-120 -- a DEVIATION of the default from the reference,
        chosen so that the benchmarked kernel is the one an API user gets; FITS files carry float64 SCI images
        either way) or uint16 reads (out_dtype=np.uint16, CLI --uint16-reads: the float32 read rounded half to even
        and saturated to 0 .. 65535 in the kernel's store -- the ADC's 16-bit unsigned DN of a real _raw file, which
        the FITS files then carry as BITPIX 16 / BZERO 32768 images; any other dtype: ValueError); `reference_quirks` keeps the reference's -5 px frame
        offset at SUBARRAY=1024 (exposure_generator.py:630) and flat-fields G102 exposures with the
        G141 cube as the reference does (grism.py:428,453-454); `record`, if a dict,
        receives the device's intermediate products (counts, x, y per bin and
        sub-sample; electrons accumulated per read interval) for parity tests;
        `exact_samplers` evaluates the per-pixel Poisson / normal draws with IEEE
        divide / sqrt and accurate log / exp / sin / cos instead of the hardware
        approximations (same algorithm and streams; for parity runs); `contaminants` -- field stars whose first-order
        spectra land on the same exposure (a list of sources.Contaminant; staring_frame passes it on too);
        `charge_traps` -- per-pixel charge trapping, the ramp effect (traps.ExposureTraps: the model with this exposure's
        start tables from its visit, as Observation.setup_charge_traps passes them; or a traps.ChargeTraps alone, whose
        traps then start every pixel at `initial`); `extraction` -- column spectra formed on the device behind the reads
        (extraction.Extraction: a plan as it is; True or an extraction.ExtractionOptions: the default plan for this
        exposure's star position and scan; staring_frame passes it on too): the returned Exposure then carries
        `spectra` [R + 1, S] and `sky` [R + 1] beside its reads; `crrej` -- cosmic-ray rejection of that extraction
        (True or an extraction.CosmicRejection; it replaces the `crrej` the extraction carries): the Exposure then
        carries `rejected` [R + 1] too; `channels` -- wavelength-binned, flat-fielded channel fluxes of that extraction
        (an extraction.Channels; it replaces the `channels` the extraction carries, with the rows' wavelength solution
        planned for this exposure): the Exposure then carries `channels` [R + 1, C] too; `variance` -- variances of that
        extraction (True or an extraction.Variances; it replaces the `variance` the extraction carries): the Exposure
        then carries `spectra_var` [R + 1, S], `sky_var` [R + 1] and, with channels, `channels_var` [R + 1, C] too;
        `optimal` -- the optimal (profile-weighted) extraction on top of those variances (True or an extraction.Optimal; it
        replaces the `optimal` the extraction carries): the Exposure then carries `optimal` and `optimal_var` [R + 1, S] too;
        `expected` -- "counts" or "mean": the noise-free expected image of the thrower stage is rendered beside the
        exposure (k_expect; wayne_hip.h, wayne_exposure_set_expected) and the Exposure carries it as `expected`
        [R, S, S] float64, electrons per read interval: what the Monte-Carlo throwers converge to, given the bin counts
        this run drew ("counts") or before the draw ("mean").  Not in it: sky, cosmic rays, dark, the gaussian-noise
        stage, gain, non-linearity, traps.  Not in replay mode.  staring_frame passes it on too;
        `ramp_fit` -- True or a rampfit.RampFit: every pixel's up-the-ramp samples are fitted with a line on the device
        (k_ramp_fit; wayne_hip.h, wayne_exposure_set_rampfit) and the Exposure carries `rate`, `rate_var` [S, S] float64
        (e-/s), `rate_word` and the derived `rate_dq`, `rate_nsamp` and `rate_time`.  The product of a STARING exposure:
        with the jump test on, a scan's trace is flagged as cosmic rays.  staring_frame passes it on too;
        `ima` -- True, "rate", "counts" or an ima.Ima: the device also forms the calibrated reads, the SCI, ERR and DQ
        arrays of an `_ima` file (k_ima; wayne_hip.h, wayne_exposure_set_ima), and the Exposure carries them as `ima`, an
        ima.Payload: the file's bytes with sci(k) / err(k) / dq(k) views.  With `ramp_fit` too, the reads behind a jump
        carry 8192 -- in a scan with the jump test on that is the trace itself.  staring_frame passes it on too;
        `ipc` -- an ipc.InterpixelCapacitance, or True for its default kernel: the electrons each read interval collected
        are coupled into the neighbouring pixels on the device, in front of the ramp kernel (k_ipc; wayne_hip.h,
        wayne_exposure_set_ipc; the law and its limits: wayne_amd/ipc.py).  Not in replay mode.  staring_frame passes it
        on too.
        """
        eng, desc, start_time = self._host_half(
            x_ref, y_ref, x_jitter, y_jitter, wl, stellar_flux, planet_signal, scan_speed, sample_rate,
            sample_mid_points, sample_durations, read_index, ssv_generator, noise_mean, noise_std, add_dark,
            add_flat, cosmic_rate, sky_background, scale_factor, add_gain_variations, add_non_linear,
            clip_values_det_limits, add_read_noise, add_stellar_noise, add_initial_bias, progress_bar, threads,
            rng_mode, out_dtype, reference_quirks, exact_samplers, contaminants, charge_traps, extraction, crrej, channels, variance, optimal,
            expected=expected, ramp_fit=ramp_fit, ima=ima, ipc=ipc)
        if record is None and desc._extraction is None and desc._expected is None and desc._ramp_fit is None and desc._ima is None:
            reads = eng.ctx.synthesize(desc)
        else:
            eng.ctx.upload(0, desc)
            eng.ctx.run_front(0)
            if record is not None:
                record["counts"], record["x"], record["y"], record["acc"] = eng.ctx.debug_fetch(0, acc=True)
                record.update(self._host_vectors)
            eng.ctx.run_back(0)
            reads = eng.ctx.download(0)
        frame = self._fill_exposure(reads, start_time)
        if desc._extraction is not None:
            spectra, sky = eng.ctx.download_spectra(0)
            self._fill_spectra(spectra, sky, eng.ctx.rejected(0) if desc._extraction.crrej is not None else None,
                               eng.ctx.channels(0) if desc._extraction.channels is not None else None,
                               eng.ctx.variances(0) if desc._extraction.variance is not None else None,
                               eng.ctx.optimal(0) if desc._extraction.optimal is not None else None,
                               eng.ctx.profile_planes(0) if eng.ctx.delivers_profile(0) else None,
                               eng.ctx.optimal_channels(0) if eng.ctx.has_optimal_channels(0) else None)
        if desc._expected is not None:
            frame.expected = eng.ctx.expected(0)
        if desc._ramp_fit is not None:
            _rampfit.fill_exposure(frame, eng.ctx.rampfit(0), self._read_dt)
        if desc._ima is not None:
            frame.ima = eng.ctx.ima(0)
        return frame

    def _fill_spectra(self, spectra, sky, rejected=None, channels=None, variances=None, optimal=None, profile_planes=None,
                      channels_opt=None):
        """The device's extraction of this generator's exposure -> Exposure.spectra [R + 1, S] / Exposure.sky [R + 1]
        (and Exposure.extraction, the plan they were formed with; Exposure.rejected [R + 1] when it rejects cosmic
        rays; Exposure.channels [R + 1, C] when it bins into wavelength channels; Exposure.spectra_var / .sky_var /
        .channels_var -- the last None without channels -- when it delivers variances; Exposure.optimal / .optimal_var
        when it extracts optimally too; Exposure.profile_planes [sum of the window heights, S] when that extraction
        delivers its profile planes)."""
        self.exposure.spectra, self.exposure.sky = spectra, sky
        self.exposure.extraction = self.extraction_plan
        if rejected is not None:
            self.exposure.rejected = rejected
        if channels is not None:
            self.exposure.channels = channels
        if variances is not None:
            self.exposure.spectra_var, self.exposure.sky_var, self.exposure.channels_var = variances
        if optimal is not None:
            self.exposure.optimal, self.exposure.optimal_var = optimal
        if profile_planes is not None:
            self.exposure.profile_planes = profile_planes
        if channels_opt is not None:               # Exposure.channels_opt / .channels_opt_var [R + 1, C]: the optimal channels
            self.exposure.channels_opt, self.exposure.channels_opt_var = channels_opt
        return self.exposure

    def _fill_exposure(self, reads, start_time=None):
        """The reads of this generator's descriptor -> its Exposure (the arrays are kept, not copied); `start_time`:
        when the exposure's generation began, for the header's SIM-TIME (None: left as it is)."""
        # read 0 is the zero read (:301-303); reads 1..R carry their timing (:371-382)
        R = len(self.read_times)
        read_dt = self._read_dt
        self.exposure.add_read(reads[0], {"cumulative_exp_time": 0.0, "read_exp_time": 0.0, "CRPIX1": 0})
        for r in range(R):
            self.exposure.add_read(reads[r + 1], {"cumulative_exp_time": float(self.read_times[r]),
                                                  "read_exp_time": float(read_dt[r]), "CRPIX1": 0})
        assert len(self.exposure.reads) == self.NSAMP                                  # (:397)
        if start_time is not None:
            self.exp_info["sim_time"] = time.time() - start_time
        return self.exposure

    def _fill_stored(self, payload, layout, start_time=None):
        """The FITS words of this generator's descriptor (device_fits: _lib.Context.wait_fits and its layout) -> its
        Exposure, holding every read as a stored piece -- views of `payload`, nothing copied: the payload must stay
        untouched until the file is written."""
        from . import fits_delivery
        R = len(self.read_times)
        S = (1014 if self.SUBARRAY == 1024 else self.SUBARRAY) + 10
        code = "u2" if layout[2] == 16 else "f8"
        pieces = fits_delivery.stored_pieces(payload, layout, R + 1)      # plane f holds read R - f
        self.exposure.add_stored_read(pieces[R], {"cumulative_exp_time": 0.0, "read_exp_time": 0.0, "CRPIX1": 0}, (S, S), code)
        for r in range(R):
            self.exposure.add_stored_read(pieces[R - 1 - r], {"cumulative_exp_time": float(self.read_times[r]),
                                                              "read_exp_time": float(self._read_dt[r]), "CRPIX1": 0}, (S, S), code)
        assert len(self.exposure.stored) == self.NSAMP
        if start_time is not None:
            self.exp_info["sim_time"] = time.time() - start_time
        return self.exposure

    def _host_half(self, x_ref, y_ref, x_jitter, y_jitter, wl, stellar_flux, planet_signal,
                   scan_speed, sample_rate, sample_mid_points=None, sample_durations=None,
                   read_index=None, ssv_generator=None, noise_mean=False, noise_std=False,
                   add_dark=True, add_flat=True, cosmic_rate=None, sky_background=1.0,
                   scale_factor=None, add_gain_variations=True, add_non_linear=True,
                   clip_values_det_limits=True, add_read_noise=True, add_stellar_noise=True,
                   add_initial_bias=True, progress_bar=None, threads=2,
                   rng_mode=_lib.RNG_SPLIT, out_dtype=np.float32, reference_quirks=False,
                   exact_samplers=False, contaminants=None, charge_traps=None, extraction=None,
                       crrej=None, channels=None, variance=None, optimal=None, device_fits=False, expected=None, ramp_fit=None, ima=None, ipc=None):
        """scanning_frame's arguments -> (engine, descriptor, start time): the mode's engine (cached after its first
        use) and build_descriptor.  No GPU call once the engine exists."""
        start_time = time.time()
        eng = _engine.get_engine(self.device, self.grism, self.detector, self.calibration, self.NSAMP,
                                 self.SAMPSEQ, self.SUBARRAY, add_initial_bias, g102_flat_quirk=reference_quirks)
        desc = self.build_descriptor(
            eng, x_ref, y_ref, x_jitter, y_jitter, wl, stellar_flux, planet_signal, scan_speed, sample_rate,
            sample_mid_points, sample_durations, read_index, ssv_generator, noise_mean, noise_std, add_dark,
            add_flat, cosmic_rate, sky_background, scale_factor, add_gain_variations, add_non_linear,
            clip_values_det_limits, add_read_noise, add_stellar_noise, add_initial_bias, progress_bar, threads,
            rng_mode, out_dtype, reference_quirks, exact_samplers, contaminants, charge_traps, extraction, crrej, channels, variance, optimal,
            device_fits=device_fits, expected=expected, ramp_fit=ramp_fit, ima=ima, ipc=ipc)
        return eng, desc, start_time

    def prepare(self, *args, staring=False, **kw):
        """The HOST half of a scanning (or, with `staring`, a staring) frame -- same arguments -- and nothing else:
        sample timing, scan positions, jitter draws, the descriptor.  It may run on another thread than the one that
        owns the context (pipeline.run_pipelined): `_prepared` = (engine, descriptor, start time) is what that thread
        uploads and runs, and _fill_exposure turns its reads into the Exposure."""
        if staring:
            args, kw = self._staring_as_scan(*args, **kw)
        self._prepared = self._host_half(*args, **kw)
        return self

    def build_descriptor(self, eng, x_ref, y_ref, x_jitter, y_jitter, wl, stellar_flux, planet_signal,
                         scan_speed, sample_rate, sample_mid_points=None, sample_durations=None,
                         read_index=None, ssv_generator=None, noise_mean=False, noise_std=False,
                         add_dark=True, add_flat=True, cosmic_rate=None, sky_background=1.0,
                         scale_factor=None, add_gain_variations=True, add_non_linear=True,
                         clip_values_det_limits=True, add_read_noise=True, add_stellar_noise=True,
                         add_initial_bias=True, progress_bar=None, threads=2,
                         rng_mode=_lib.RNG_SPLIT, out_dtype=np.float32, reference_quirks=False,
                         exact_samplers=False, contaminants=None, charge_traps=None, extraction=None,
                       crrej=None, channels=None, variance=None, optimal=None, device_fits=False, expected=None, ramp_fit=None, ima=None, ipc=None):
        """The host half of scanning_frame: sample timing, scan positions, SSV,
        jitter / seed draws, spectrum crop (exposure_generator.py:247-334) ->
        one wayne_exposure_desc for the device.  Pure host code (`eng` may be
        None when no GPU is involved, e.g. when sharding a visit on the CPU).
        `device_fits`: Context.upload also asks the device for the reads' FITS words (wayne_exposure_set_fits), the way
        it applies `extraction`; nothing the device computes for the reads changes.  `expected`: "counts" or "mean" --
        Context.upload also asks for the noise-free expected image (wayne_exposure_set_expected); refused here, with a
        ValueError, for any other value and in replay mode.  `ramp_fit`: True or a rampfit.RampFit -- Context.upload also
        asks for the ramp fit (wayne_exposure_set_rampfit).  `ima`: True, "rate", "counts" or an ima.Ima -- Context.upload
        also asks for the calibrated reads (wayne_exposure_set_ima).  `ipc`: an ipc.InterpixelCapacitance or True --
        Context.upload also asks for the inter-pixel capacitance (wayne_exposure_set_ipc); refused here in replay mode."""
        ipc = _ipc.as_ipc(ipc)
        if ipc is not None and rng_mode == _lib.RNG_REPLAY:
            raise ValueError("ipc: replay mode reproduces the reference, which has no inter-pixel capacitance")
        if _lib.expected_mode(expected) and rng_mode == _lib.RNG_REPLAY:
            raise ValueError("expected: replay mode reproduces the reference, which has no expected image")
        out_dtype = np.dtype(out_dtype)
        if out_dtype not in _lib.OUT_FLAGS:
            raise ValueError("out_dtype must be float32, float64 or uint16, not %s" % out_dtype)
        wl = np.asarray(wl, dtype=float)
        stellar_flux = np.asarray(stellar_flux, dtype=float)
        scan_speed_ms = scan_speed / 1000.          # px/s -> px/ms (:247)

        if sample_mid_points is None and sample_durations is None and read_index is None:
            _, sample_mid_points, sample_durations, read_index = self._gen_scanning_sample_times(sample_rate)
        sample_mid_points = np.asarray(sample_mid_points, dtype=float)
        sample_durations = np.asarray(sample_durations, dtype=float)

        s_y_refs = self._gen_sample_yref(y_ref, sample_mid_points, scan_speed_ms)     # (:258)
        if ssv_generator is not None:
            if isinstance(ssv_generator, scan_speed_varations.SSVModulatedSine):          # (:263-267)
                # its scalar draws are keyed by (visit seed, exposure): order-independent
                ssv_generator.rng_seed = (self.seed * 1000003 + self.exposure_index * 7919 + 12345) & 0x7FFFFFFF
                sample_durations, read_index = ssv_generator.get_subsample_exposure_times(
                    s_y_refs, sample_durations, self.read_times, sample_rate)
                sample_durations = np.asarray(sample_durations, dtype=float)
                # it yields len(tt) durations; samples without one expose for 0 ms (:337-342)
                read_index = [min(int(b), len(sample_mid_points) - 1) for b in read_index]
                read_index[-1] = len(sample_mid_points) - 1
            else:
                sample_durations = np.asarray(ssv_generator.get_subsample_exposure_times(
                    s_y_refs, sample_durations, self.read_times, sample_rate), dtype=float)   # (:272-273)

        self.exp_info.update({
            "SCAN": True, "SCAN_DIR": 1, "samp_rate": sample_rate, "x_ref": x_ref, "y_ref": y_ref,
            "noise_mean": noise_mean, "noise_std": noise_std, "add_dark": add_dark, "add_flat": add_flat,
            "add_gain": add_gain_variations, "add_non_linear": add_non_linear,
            "add_stellar_noise": add_stellar_noise, "cosmic_rate": cosmic_rate,
            "sky_background": sky_background, "scale_factor": scale_factor,
            "clip_values_det_limits": clip_values_det_limits,
        })
        if contaminants:
            self.exp_info["contaminants"] = list(contaminants)     # (the FITS header names them: exposure.py)
        else:
            self.exp_info.pop("contaminants", None)
        charge_traps = _traps.for_exposure(charge_traps)
        if charge_traps is not None:
            self.exp_info["charge_traps"] = charge_traps.traps     # (the FITS header records the model: exposure.py)
        else:
            self.exp_info.pop("charge_traps", None)
        if ipc is not None:
            self.exp_info["interpixel_capacitance"] = ipc          # (the FITS header records the weights: exposure.py)
        else:
            self.exp_info.pop("interpixel_capacitance", None)
        self.exposure = exposure.Exposure(self.detector, self.grism, self.planet, self.exp_info)

        if add_dark and eng is not None and not eng.has_dark:
            # the reference switches the dark off with a warning when the mode has no super-dark (:414-423)
            warnings.warn("No Dark file found for SAMPSEQ = {}, SUBARRAY={} - Switching Dark Off".format(
                self.SAMPSEQ, self.SUBARRAY), WFC3SimNoDarkFileWarning)
            add_dark = False
            self.exposure.exp_info["add_dark"] = False

        K = len(sample_mid_points)
        R = len(self.read_times)
        # per-exposure draws (:327-329): replay seeds and per-sub-sample jitter
        z_x, z_y, s_rand_seeds = _lib.host_sample_draws(self.seed, self.exposure_index, K)
        s_x = x_ref + z_x * x_jitter
        s_y_refs = np.asarray(s_y_refs, dtype=float)
        s_y = s_y_refs[np.minimum(np.arange(K), len(s_y_refs) - 1)] + z_y * y_jitter
        # a sub-sample without a duration (bad SSV) exposes for 0 ms (:337-342)
        s_dur = np.zeros(K)
        n_dur = min(K, len(sample_durations))
        s_dur[:n_dur] = np.asarray(sample_durations, dtype=float)[:n_dur]

        # crop to the grism's limits (:332-334); every exposure of a visit brings the same grid: looked up once
        key = (wl.size, float(wl[0]), float(wl[-1]), float(wl[wl.size // 2]), self.grism.wl_limits[0],
               self.grism.wl_limits[-1])
        hit = _CROP_CACHE.get(key)
        if hit is None or not np.array_equal(hit[0], wl):
            if len(_CROP_CACHE) > 16:
                _CROP_CACHE.clear()
            hit = _CROP_CACHE[key] = (wl.copy(), tools.crop_spectrum_ind(self.grism.wl_limits[0],
                                                                         self.grism.wl_limits[-1], wl))
        i0, i1 = hit[1]
        s_wl = wl[i0:i1]
        flux = stellar_flux[i0:i1]
        depth = None
        lc = {}
        if isinstance(planet_signal, lightcurve.DeviceDepths):
            # the K x W matrix is computed on the device from K + W + 4 numbers
            with np.errstate(invalid="ignore"):      # (a negative element: NaN, a column without a planet -- k_lightcurve)
                rp = np.sqrt(planet_signal.planet_spectrum[i0:i1])
            lc = dict(lc_z=planet_signal.z_tr, lc_hidden=planet_signal.hidden, lc_rp=rp, lc_ld=planet_signal.ld)
            if getattr(planet_signal, "ld_table", None) is not None:     # coefficients per bin: cropped with the spectrum
                lc["lc_ld_table"] = planet_signal.ld_table[i0:i1]
            if getattr(planet_signal, "spots", None) is not None:        # star spots: their contrast likewise
                lc["lc_spots"] = planet_signal.spots.crop(i0, i1)
        elif planet_signal is not None:
            depth = np.ascontiguousarray(np.asarray(planet_signal, dtype=float)[:, i0:i1])

        # the read that closes each sub-sample (`if i in read_index`, :361)
        read_index = list(read_index)
        if len(read_index) != R or read_index[-1] != K - 1:
            raise ValueError("read_index must name the last sub-sample of each of the %d reads" % R)
        sample_read = np.searchsorted(np.asarray(read_index), np.arange(K), side="left").astype(np.int32)
        read_dt = np.diff(np.concatenate([[0.0], self.read_times]))                   # (:362-365)

        flags = 0
        for on, bit in ((add_flat, _lib.F_ADD_FLAT), (add_gain_variations, _lib.F_ADD_GAIN_VARIATIONS),
                        (add_non_linear, _lib.F_ADD_NON_LINEAR), (clip_values_det_limits, _lib.F_CLIP_DET_LIMITS),
                        (add_read_noise, _lib.F_ADD_READ_NOISE), (add_stellar_noise, _lib.F_ADD_STELLAR_NOISE),
                        (add_dark, _lib.F_ADD_DARK), (add_initial_bias, _lib.F_ADD_INITIAL_BIAS),
                        (True, _lib.OUT_FLAGS[out_dtype]),
                        (exact_samplers, _lib.F_EXACT_SAMPLERS)):
            if on:
                flags |= bit
        # frame offset 507 - SUBARRAY/2 (:630).  At 1024 the reference gets -5,
        # which shifts the spectrum by +5 px on a 1014 frame: use 0.
        sub_scale = 507 - self.SUBARRAY // 2
        if self.SUBARRAY == 1024 and not reference_quirks:
            sub_scale = 0

        if eng is not None:
            eng.check_descriptor(sub_scale)
        S = (1014 if self.SUBARRAY == 1024 else self.SUBARRAY) + 10
        self.extraction_plan = _extraction.for_exposure(extraction, self.grism, s_wl, x_ref, y_ref, scan_speed,
                                                        self.read_times, sub_scale, S, crrej, channels, variance, optimal)
        # what exposures must share to share a profile of the optimal extraction (extraction.profile_key)
        self.profile_key = None if self.extraction_plan is None else _extraction.profile_key(self.extraction_plan, scan_speed)
        self._read_dt = read_dt
        self._host_vectors = {"x_ref": s_x, "y_ref": s_y, "dur": s_dur, "seeds": s_rand_seeds, "read": sample_read}
        return _lib.make_desc(
            self.seed, self.exposure_index, flags, sub_scale, s_wl, flux, depth, s_x, s_y, s_dur,
            sample_read, read_dt, replay_seed=s_rand_seeds, rng_mode=rng_mode, threads_compat=threads,
            sky_ct_s=float(sky_background) if sky_background else 0.0,
            cosmic_rate=-1.0 if cosmic_rate is None else float(cosmic_rate),
            scale_factor=1.0 if scale_factor is None else float(scale_factor),
            noise_mean=float(noise_mean) if noise_mean else 0.0,
            noise_std=float(noise_std) if noise_std else 0.0, sources=contaminants, traps=charge_traps,
            extraction=self.extraction_plan, device_fits=device_fits, expected=expected, ramp_fit=ramp_fit, ima=ima, ipc=ipc, **lc)

    def direct_image(self, x_ref, y_ref):
        """The unscaled 2-D gaussian direct image used to calibrate x_ref / y_ref
        (exposure_generator.py:83-144): zero read + one read, no detector effects."""
        self.exp_info.update({"OBSTYPE": "IMAGING", "x_ref": x_ref, "NSAMP": 2, "SAMP-SEQ": "RAPID",
                              "y_ref": y_ref, "add_flat": False, "add_gain": False, "add_non_linear": False,
                              "add_read_noise": False, "cosmic_rate": 0, "sky_background": 0.0,
                              "scale_factor": 1, "clip_values_det_limits": False})
        self.exposure = exposure.Exposure(self.detector, None, self.planet, self.exp_info)
        self.exposure.add_read(self.detector.gen_pixel_array(self.SUBARRAY, light_sensitive=False))
        n = self.SUBARRAY
        x, y = np.meshgrid(np.arange(n, dtype=float) + 0.5, np.arange(n, dtype=float) + 0.5)
        x0 = x_ref - (507.0 - n / 2.0)
        y0 = y_ref - (507.0 - n / 2.0)
        sigma = 2.0
        di = 10000.0 * np.exp(-((x0 - x) ** 2 + (y0 - y) ** 2) / (2.0 * sigma * sigma))
        self.exposure.add_read(di, {"read_exp_time": 0.0, "cumulative_exp_time": 0.0, "CRPIX1": -5})
        return self.exposure
