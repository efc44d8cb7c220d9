"""Running a visit: exposures sharded round-robin over GPUs, one process per GPU.

Exposures of a visit share no state (the reference only couples them through
its sequential global RNG, observation.py:403-405, which the Philox counters
remove), so exposure i goes to rank i mod G with no collective in the data
path.  Each rank owns one Engine (context + resident
calibration) and writes its own NNNN_raw.fits files (observation.py:427).
"""
import hashlib
import os

import numpy as np

from . import _lib
from . import engine as _engine
from . import extraction as _extraction
from .expected import ExpectedDelivery
from . import rampfit as _rampfit
from . import ima as _ima
from . import ipc as _ipc
from .exposure import FitsWriterPool
from .exposure_generator import ExposureGenerator
from .fits_delivery import FitsDelivery, slots_for
from .pipeline import run_pipelined


def shard(n_exposures, rank, world):
    """Exposure indices of `rank`: i = rank, rank + world, ... (round-robin keeps
    orbit phase, and so per-exposure cost, balanced across ranks)."""
    if not 0 <= rank < world:
        raise ValueError("rank %d outside world %d" % (rank, world))
    return list(range(rank, n_exposures, world))


def descriptor_digest(desc):
    """SHA-1 over everything a descriptor hands to the device (for sharding tests)."""
    h = hashlib.sha1()
    for name, _ in desc._fields_:
        v = getattr(desc, name)
        if isinstance(v, (int, float)):
            h.update(repr((name, v)).encode())
    for a in desc._keep:
        h.update(np.ascontiguousarray(a).tobytes())
    for src in getattr(desc, "_sources", ()):      # contaminants (none: the digest of a descriptor without them)
        h.update(src.digest_bytes())
    traps = getattr(desc, "_traps", None)          # charge traps (none: likewise)
    if traps is not None:
        h.update(traps.digest_bytes())
    ld_table = getattr(desc, "_ld_table", None)    # limb darkening per wavelength bin (none: likewise)
    if ld_table is not None:
        h.update(b"ld_table" + np.ascontiguousarray(ld_table).tobytes())
    lc_spots = getattr(desc, "_spots", None)       # star spots of the device light curve (none: likewise)
    if lc_spots is not None:
        h.update(lc_spots.digest_bytes())
    ipc = getattr(desc, "_ipc", None)              # inter-pixel capacitance (none: likewise)
    if ipc is not None:
        h.update(ipc.digest_bytes())
    return h.hexdigest()


class VisitRunner(object):
    """Generate the exposures `indices` of a synthetic.Visit-like object on one GPU."""

    # exposures in flight: slots 0..DEPTH-1 in rotation, alternating over the context's two streams (an even number
    # keeps the streams balanced; scripts/probe_pipeline.py: 2 -> 826 /s, 3 -> 646, 4 -> 809 for resident descriptors)
    DEPTH = 4

    def __init__(self, visit, device=0, out_dir=None, out_dtype=np.float32, frame_overrides=None, device_lc=False,
                 device_fits=False, ipc=None):
        """`device_lc`: hand the device the K + W + 4 numbers of the light-curve model (visit.device_depths)
        instead of a K x W transit-depth matrix computed on the host.  `device_fits`: the device forms the files' data
        sections and `run` writes each file straight from the slot's pinned mirror (fits_delivery): the same files.
        `ipc`: an ipc.InterpixelCapacitance, or True for its default kernel -- every exposure's collected charge is
        coupled into the neighbouring pixels on the device (wayne_amd/ipc.py); None: none."""
        self.visit, self.device, self.out_dir = visit, device, out_dir
        self.ipc = _ipc.as_ipc(ipc)
        self.out_dtype = out_dtype
        self.frame_overrides = frame_overrides or {}
        self.device_lc = device_lc
        self.device_fits = bool(device_fits)
        self.rng_mode = 2            # WAYNE_RNG_SPLIT
        self._eng = None

    def engine(self):
        if self._eng is None:
            v = self.visit
            self._eng = _engine.get_engine(self.device, v.grism, v.detector, v.calibration, v.NSAMP, v.SAMPSEQ,
                                           v.SUBARRAY,
                                           g102_flat_quirk=bool(self.frame_overrides.get("reference_quirks", False)))
        return self._eng

    def generator(self, i):
        v = self.visit
        return ExposureGenerator(v.detector, v.grism, v.NSAMP, v.SAMPSEQ, v.SUBARRAY, calibration=v.calibration,
                                 device=self.device, seed=v.seed, exposure_index=i,
                                 filename="%04d_raw.fits" % (i + 1))

    def frame_kwargs(self, i):
        over = dict(self.frame_overrides)
        if self.device_lc:
            over["planet_signal"] = self.visit.device_depths(i)
        if self.ipc is not None:
            over["ipc"] = self.ipc
        return self.visit.frame_kwargs(i, **over)

    def descriptor(self, i, eng=None):
        return self.generator(i).build_descriptor(eng, out_dtype=self.out_dtype, rng_mode=self.rng_mode,
                                                  **self.frame_kwargs(i))

    def run(self, indices, keep=False, on_reads=None, extraction=None, on_spectra=None, expected=None, on_expected=None,
            ramp_fit=None, on_ramp_fit=None, ima=None, on_ima=None):
        """Synthesise the given exposures as a pipeline over the context's two HIP streams and pinned
        host buffers: while the kernels of exposure n run on one stream and the device-to-host copy of
        exposure n-1 on the other, the host prepares and uploads exposure n+1 into the next slot.
        `on_reads(i, reads)` is called with a view of the pinned buffer (copy it to keep it);
        keep=True returns {index: copy}; FITS files are written when out_dir is set.
        `extraction` (True, an extraction.ExtractionOptions, or one extraction.Extraction for every exposure): the
        device extracts each exposure's column spectra behind its reads and both are delivered --
        `on_spectra(i, spectra, sky)` gets views of the pinned buffer, and keep=True returns
        {index: (reads, spectra, sky)}.  When the extraction delivers variances, `self.spectra_var`, `self.sky_var` and
        -- with channels -- `self.channels_var` are {index: array} of every exposure run (None otherwise); when it
        extracts optimally too, so are `self.optimal` and `self.optimal_var`, and `self.profile_planes` when it delivers
        its profile planes.  `expected` ("counts" or "mean"): every exposure's noise-free expected image is rendered
        beside it (wayne_amd/expected.py) and fetched behind its settled run: `on_expected(i, planes)` gets an array
        [R, S, S] of the caller's own, and with keep=True `self.expected` is {index: planes} (None otherwise).
        `ramp_fit` (True or a rampfit.RampFit): every exposure's ramps are fitted on the device (wayne_amd/rampfit.py) and
        the planes fetched behind its settled run: `on_ramp_fit(i, rate, var, word)` gets arrays [S, S] of the caller's
        own, with keep=True `self.ramp_fit` is {index: (rate, var, word)} (None otherwise), and with out_dir set
        NNNN_rate.fits is written beside each raw file.  `ima` (True, "rate", "counts" or an ima.Ima): every exposure's
        calibrated reads are formed on the device (wayne_amd/ima.py) and fetched behind its settled run: `on_ima(i, payload)`
        gets an ima.Payload of the caller's own, with keep=True `self.ima` is {index: payload} (None otherwise), and with
        out_dir set NNNN_ima.fits is written beside each raw file."""
        eng = self.engine()
        results = {}
        _lib.expected_mode(expected)          # (ValueError for anything but None, "counts", "mean")
        self.expected = {} if expected and keep else None
        ramp_fit = _rampfit.as_ramp_fit(ramp_fit)
        _rampfit.refuse_combinations(ramp_fit, device_fits=self.device_fits and self.out_dir is not None)
        self.ramp_fit = {} if ramp_fit is not None and keep else None
        ima = _ima.as_ima(ima)
        _ima.refuse_combinations(ima, device_fits=self.device_fits and self.out_dir is not None)
        self.ima = {} if ima is not None and keep else None
        self.spectra_var = self.sky_var = self.channels_var = None
        self.optimal = self.optimal_var = None
        self.profile_planes = None
        self.channels_opt = self.channels_opt_var = None      # {index: [R + 1, C]} when the optimal channels are formed
        pool = FitsWriterPool() if self.out_dir is not None else None
        # device_fits: the files' data sections come from the device and each file is written from its slot's pinned
        # mirror; the reads themselves are fetched only for a caller that asked for them
        fits = self.device_fits and pool is not None
        want_reads = keep or on_reads is not None

        def prepare(i):
            gen = self.generator(i)
            kw = self.frame_kwargs(i)
            if extraction is not None:
                kw["extraction"] = extraction
            if fits:
                kw["device_fits"] = True
            if expected:
                kw["expected"] = expected
            if ramp_fit is not None:
                kw["ramp_fit"] = ramp_fit
            if ima is not None:
                kw["ima"] = ima
            return gen.build_descriptor(eng, out_dtype=self.out_dtype, rng_mode=self.rng_mode, **kw), gen

        def finish(i, gen, got):
            reads = payload = got
            if fits:
                reads = ctx.reads_view
                if extraction is not None:
                    payload, spectra, sky = got
            elif extraction is not None:
                reads, spectra, sky = got
            if extraction is not None:
                if ctx.variances is not None:
                    if self.spectra_var is None:
                        self.spectra_var, self.sky_var = {}, {}
                        self.channels_var = {} if ctx.variances[2] is not None else None
                    self.spectra_var[i], self.sky_var[i] = ctx.variances[0], ctx.variances[1]
                    if self.channels_var is not None:
                        self.channels_var[i] = ctx.variances[2]
                if ctx.optimal is not None:
                    if self.optimal is None:
                        self.optimal, self.optimal_var = {}, {}
                    self.optimal[i], self.optimal_var[i] = ctx.optimal
                if ctx.channels_opt is not None:
                    if self.channels_opt is None:
                        self.channels_opt, self.channels_opt_var = {}, {}
                    self.channels_opt[i], self.channels_opt_var[i] = ctx.channels_opt
                if ctx.profile_planes is not None:
                    if self.profile_planes is None:
                        self.profile_planes = {}
                    self.profile_planes[i] = ctx.profile_planes
                if on_spectra is not None:
                    on_spectra(i, spectra, sky)
            if expected:
                if on_expected is not None:
                    on_expected(i, ctx.expected)
                if self.expected is not None:
                    self.expected[i] = ctx.expected
            if ramp_fit is not None:
                if on_ramp_fit is not None:
                    on_ramp_fit(i, *ctx.ramp_fit)
                if self.ramp_fit is not None:
                    self.ramp_fit[i] = ctx.ramp_fit
            if ima is not None:
                if on_ima is not None:
                    on_ima(i, ctx.ima)
                if self.ima is not None:
                    self.ima[i] = ctx.ima
            if on_reads is not None:
                on_reads(i, reads)
            if keep:
                results[i] = reads.copy() if extraction is None else (reads.copy(), spectra.copy(), sky.copy())
            if fits:
                os.makedirs(self.out_dir, exist_ok=True)
                # (no copy: the slot is not uploaded again until the writer has released it -- FitsDelivery.lease)
                pool.submit(gen._fill_stored(payload, ctx.layout), self.out_dir, gen.exp_info["filename"], done=ctx.lease())
            elif pool is not None:
                os.makedirs(self.out_dir, exist_ok=True)
                # (a copy: the pinned buffer is reused by the next exposure)
                frame = gen._fill_exposure(reads.copy())
                if ramp_fit is not None:
                    # (written here, beside the raw file the pool writes: the header's clock aside, a function of the planes)
                    _rampfit.fill_exposure(frame, ctx.ramp_fit, gen._read_dt)
                    _rampfit.write_fits(os.path.join(self.out_dir, _rampfit.rate_filename(gen.exp_info["filename"])), frame, ramp_fit)
                if ima is not None:
                    frame.ima = ctx.ima
                    _ima.write_fits(os.path.join(self.out_dir, _ima.ima_filename(gen.exp_info["filename"])), frame)
                pool.submit(frame, self.out_dir, gen.exp_info["filename"])

        n_slots = self.DEPTH
        if fits:
            inner = None if extraction is None else _extraction.Delivery(eng.ctx, reads=want_reads)
            ctx = FitsDelivery(eng.ctx, extraction=inner, reads=want_reads)
            n_slots = slots_for(self.DEPTH, pool.n_threads)
        else:
            ctx = eng.ctx if extraction is None else _extraction.Delivery(eng.ctx, reads=True)
        if expected:
            ctx = ExpectedDelivery(eng.ctx, ctx)
        if ramp_fit is not None:
            ctx = _rampfit.RampFitDelivery(eng.ctx, ctx)
        if ima is not None:
            ctx = _ima.ImaDelivery(eng.ctx, ctx)
        try:
            run_pipelined(ctx, indices, prepare, finish, self.DEPTH, n_slots)
        finally:
            if pool is not None:
                pool.close()
        return results

    def run_spectra(self, indices, extraction=True):
        """The same pipeline with only the spectra delivered: every exposure is synthesised and extracted on the device
        (`extraction`: as in run) and 8 (R + 1)(S + 1) bytes of it reach the host -- the reads never leave the device.
        -> (spectra [n, R + 1, S], sky [n, R + 1]) in the order of `indices`; `self.plans` [n]: each exposure's
        extraction.Extraction; `self.rejected` [n, R + 1]: the flag counts of an extraction that rejects cosmic rays
        (None otherwise); `self.channels` [n, R + 1, C]: the channel fluxes of an extraction that bins into wavelength
        channels (None otherwise); `self.spectra_var` [n, R + 1, S], `self.sky_var` [n, R + 1] and -- with channels --
        `self.channels_var` [n, R + 1, C]: the variances of an extraction that delivers them (None otherwise);
        `self.optimal` and `self.optimal_var` [n, R + 1, S]: the optimal extraction's, when asked for (None otherwise);
        `self.profile_planes` [n] arrays [sum of the exposure's window heights, S]: its profile planes, when the optimal
        extraction delivers them (None otherwise)."""
        eng = self.engine()
        indices = list(indices)
        where = {i: n for n, i in enumerate(indices)}
        R, S = eng.ctx.R, eng.ctx.S
        spectra = np.empty((len(indices), R + 1, S))
        sky = np.empty((len(indices), R + 1))
        self.plans = [None] * len(indices)
        counts = [None] * len(indices)
        binned = [None] * len(indices)
        varis = [None] * len(indices)
        optis = [None] * len(indices)
        planes = [None] * len(indices)
        keys = [None] * len(indices)
        optch = [None] * len(indices)
        delivery = _extraction.Delivery(eng.ctx, reads=False)

        def prepare(i):
            gen = self.generator(i)
            kw = self.frame_kwargs(i)
            kw["extraction"] = extraction
            return gen.build_descriptor(eng, out_dtype=self.out_dtype, rng_mode=self.rng_mode, **kw), gen

        def finish(i, gen, got):
            _, sp, sk = got
            spectra[where[i]], sky[where[i]] = sp, sk
            self.plans[where[i]] = gen.extraction_plan
            counts[where[i]] = delivery.rejected
            binned[where[i]] = delivery.channels
            varis[where[i]] = delivery.variances
            optis[where[i]] = delivery.optimal
            planes[where[i]] = delivery.profile_planes
            keys[where[i]] = gen.profile_key
            optch[where[i]] = delivery.channels_opt

        run_pipelined(delivery, indices, prepare, finish, self.DEPTH, self.DEPTH)
        self.rejected = None if any(n is None for n in counts) or not counts else np.array(counts, dtype=np.uint32)
        self.channels = None if any(c is None for c in binned) or not binned else np.array(binned, dtype=np.float64)
        self.spectra_var = self.sky_var = self.channels_var = None
        if varis and not any(v is None for v in varis):
            self.spectra_var = np.array([v[0] for v in varis], dtype=np.float64)
            self.sky_var = np.array([v[1] for v in varis], dtype=np.float64)
            if not any(v[2] is None for v in varis):
                self.channels_var = np.array([v[2] for v in varis], dtype=np.float64)
        self.optimal = self.optimal_var = None
        if optis and not any(o is None for o in optis):
            self.optimal = np.array([o[0] for o in optis], dtype=np.float64)
            self.optimal_var = np.array([o[1] for o in optis], dtype=np.float64)
        self.profile_planes = planes if planes and not any(a is None for a in planes) else None
        self.profile_keys = keys          # [n] extraction.profile_key of each exposure
        self.channels_opt = self.channels_opt_var = None      # [n, R + 1, C]: the optimal channels, when asked for
        if optch and not any(o is None for o in optch):
            self.channels_opt = np.array([o[0] for o in optch], dtype=np.float64)
            self.channels_opt_var = np.array([o[1] for o in optch], dtype=np.float64)
        return spectra, sky

    def build_profile(self, indices, extraction):
        """The visit's profiles for the optimal extraction: the exposures `indices` are run with `extraction` (an
        ExtractionOptions or Extraction with variances and optimal) and their profile planes delivered, added up and
        normalised -> {(window heights [R + 1], scan direction +1 / -1 / 0): extraction.Profile}, one per distinct key
        (forward and reverse scans illuminate the rows in opposite order; exposures whose windows differ in height cannot
        share planes)."""
        indices = list(indices)
        if getattr(extraction, "optimal", None) is None:
            raise ValueError("build_profile: the extraction must carry optimal=")
        self.run_spectra(indices, extraction=extraction.with_optimal(extraction.optimal.with_profile(None, deliver_profile=True, channels=False)))
        sums = {}
        for key, plan, planes in zip(self.profile_keys, self.plans, self.profile_planes):
            sums.setdefault(key, _extraction.ProfileSum()).add(plan, planes)
        return {key: acc.profile() for key, acc in sums.items()}

    def run_resident_spectra(self, n, on_spectra=None):
        """run_resident with only the spectra delivered: the descriptors AND their extraction are already in slots
        0..DEPTH-1; n exposures, kernels + extraction + the copy of the spectra block, no reads copied."""
        ctx = self.engine().ctx
        pending = []

        def done(s_old):
            spectra, sky = ctx.wait_spectra(s_old)
            if on_spectra is not None:
                on_spectra(s_old, spectra, sky)

        for j in range(n):
            slot = j % self.DEPTH
            if len(pending) == self.DEPTH:
                done(pending.pop(0))
            ctx.run(slot)
            ctx.fetch_spectra_async(slot)
            pending.append(slot)
        for s_old in pending:
            done(s_old)

    def run_resident(self, n, on_reads=None):
        """The same pipeline over descriptors that are ALREADY in slots 0..DEPTH-1 (uploaded by the
        caller): n exposures, kernels + copy to pinned host memory, no host preparation or upload."""
        ctx = self.engine().ctx
        pending = []
        for j in range(n):
            slot = j % self.DEPTH
            if len(pending) == self.DEPTH:
                s_old = pending.pop(0)
                reads = ctx.wait(s_old)
                if on_reads is not None:
                    on_reads(s_old, reads)
            ctx.run(slot)
            ctx.fetch_async(slot)
            pending.append(slot)
        for s_old in pending:
            reads = ctx.wait(s_old)
            if on_reads is not None:
                on_reads(s_old, reads)
