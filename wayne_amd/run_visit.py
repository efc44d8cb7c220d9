"""Command line: generate a visit from a YAML parameter file.

    python -m wayne_amd.run_visit -p <parameter_file> [--calibration DIR] [--device N] [--max-exposures M] [--gpus G] [--resume]
                                  [--spectra OUT.npz | --spectra-only OUT.npz] [--reject-cosmics [K]]
                                  [--channels LO:HI:N] [--no-channel-flat] [--variances [RN]] [--optimal [H]] [--optimal-profile N] [--optimal-channels]
                                  [--float64-reads | --uint16-reads] [--device-fits] [--expected {counts,mean}]
                                  [--rate-images [K]] [--ima [{rate,counts}]]

Accepts the reference's parameter files (wayne/run_visit.py:1-9, example
examples/hd209458b_12181_simulation_parameters.yml): sections `general`
(outdir, seed, threads), `target`, `observation`, `trends`.  Differences:

  * calibration files come from --calibration DIR (the reference downloads
    them at import, params.py:41-56); without it seeded synthetic planes are used;
  * planet parameters come from the YAML (`period`, `sma`, `stellar_radius`,
    `inclination`, `eccentricity`, `periastron`, `transit_time`, `ldcoeffs`);
    the Open Exoplanet Catalogue lookup (oec.py) is not provided;
  * a missing stellar spectrum file falls back to a black body of
    `target: star_temperature` (default 6100 K);
  * `--resume`: exposures whose files are already in the output directory (whole, and this visit's: same start time and
    mode) are skipped; files are written under a temporary name and renamed, so an interrupted run leaves no partial
    file under a final name.  A resumed visit's files are those of an uninterrupted one (per-exposure Philox keys);
  * an optional top-level `contaminants:` list puts field stars on every exposure (wayne_amd/sources.py): per entry
    `dx`, `dy` (px from the target), `flux_ratio` (detected electrons relative to the target's) and a black-body
    `temperature` or a PHOENIX `spectrum_file`; at most 8.  First order only, not in the direct image, constant;
  * an optional `target: ld_table: {law: claret4, wl_um: [...], coeffs: [[...], ...]}` or `target: ld_table_file: FILE`
    (text, columns wl_um a1 a2 a3 a4; `ld_law: quadratic | linear` for a file with wl_um u1 u2 or wl_um u) gives every
    wavelength bin its own limb darkening, interpolated linearly between the nodes (lightcurve.LimbDarkening);
    `ldcoeffs` stays required (the header's LD1 .. LD4); the files then carry LDTABLE, LDLAW, LDNODES, LDWLLO, LDWLHI, LDHASH;
  * an optional `target: spots: {photosphere_temperature: 5000, list: [{x: -0.21, y: 0.33, radius: 0.10, temperature:
    4200}, {at_phase: 0.0021, radius: 0.06, contrast: 0.75}]}` puts star spots into the light curves, occulted and
    unocculted (wayne_amd/spots.py): at most 8 circles in projection, centre and radius in stellar radii (`at_phase`:
    centred where the planet's centre is at that orbital phase from mid-transit, in periods), each with a `contrast` or
    a `temperature` (K; `photosphere_temperature` is then required); the files then carry SPOTS, NSPOTS, SPTXn, SPTYn,
    SPTRn, SPTCn and SPTHASH;
  * an optional top-level `charge_traps:` section turns on per-pixel charge trapping, the ramp effect
    (wayne_amd/traps.py): `slow` / `fast` mappings of n_traps, efficiency, lifetime_s, initial, orbit_fill; `{}` = the
    defaults, an omitted key its default; `history: carried` carries each pixel's trap state from exposure to exposure
    on the device (default `planned`) -- one rank only, no --resume;
  * an optional top-level `interpixel_capacitance:` section couples the charge each read interval collected into the
    neighbouring pixels (wayne_amd/ipc.py): `alpha: a` or `kernel: [[..],[..],[..]]`, `{}` = the default kernel; the files
    then carry IPC, IPCUNIT and IPCW00 .. IPCW22; goes with --gpus, --ranks-per-gpu, --resume and every other option;
  * `--spectra OUT.npz`: the device extracts every exposure's column spectra behind its reads (wayne_amd/extraction.py)
    and they are written to OUT.npz beside the _raw files: spectra [n, NSAMP, S], sky [n, NSAMP], exposure_index, row_lo,
    row_hi, bg_cols, x_ref, y_ref, read_times, exp_start.  `--spectra-only OUT.npz`: the same file, no _raw files, and
    the reads never leave the device.  Neither goes with --resume.  With --gpus G > 1 each rank writes its own file,
    `.rankNN` before the extension; they are not merged.  `--reject-cosmics [K]` (with either): cosmic rays are
    rejected on the difference images first, K sigma (default 8) above a pixel's stencil neighbours; OUT.npz then also
    holds n_rejected [n, NSAMP] -- the pixels replaced in each read interval's window and, last, the (pixel, interval)
    pairs corrected in the last-read product -- crrej_k and crrej_read_noise.  `--channels LO:HI:N` (with either): every
    exposure is also binned on the device into N wavelength channels of equal width between LO and HI um, each row by
    its own wavelength solution and each pixel divided by the flat cube at its wavelength (`--no-channel-flat`: not
    divided); OUT.npz then also holds channels [n, NSAMP, N], channel_edges_um [N + 1], channel_flat and the rows'
    solutions wl_a / wl_b [n, S].  `--variances [RN]` (with either): the device also sums every window pixel's variance
    -- Poisson on its own electrons plus the read noise RN of a difference of two reads (default 20 e-) through its own
    gain -- beside its flux; OUT.npz then also holds spectra_var [n, NSAMP, S], sky_var [n, NSAMP], with --channels
    channels_var [n, NSAMP, N], and variance_read_noise.  `--optimal [H]` (with --variances): the device also forms the
    optimal (profile-weighted) spectra, each column's profile taken from the window's own light over 2H + 1 columns
    (default H = 8, 1 .. 16); OUT.npz then also holds optimal, optimal_var [n, NSAMP, S] and optimal_half_width;
    `--optimal-profile N` (with --optimal): the profiles are formed once, from the first N exposures of each group, and
    OUT.npz also holds optimal_profile_exposures;
  * `--device-fits`: the device forms the data sections of the _raw files (big-endian words in file order, padding
    included) and every file is written straight from the pinned memory they are copied into: the same files, byte for
    byte, without the host's pass over the samples (wayne_amd/fits_delivery.py).  With every other option but
    --spectra-only (which writes no _raw files); the direct image stays on the host path;
  * `--expected {counts,mean}`: the device also renders every exposure's noise-free expected image (wayne_amd/expected.py:
    what the electron thrower converges to, given the bin counts the run drew -- counts -- or before the draw -- mean;
    electrons per read interval, without sky, cosmic rays, dark and the detector chain) and NNNN_exp.fits is written
    beside each _raw file: the raw file's primary header plus EXPMODE, then one image HDU EXPECT per read interval
    (EXTVER 1 .. R, BITPIX -64).  Not with --resume, --device-fits, --spectra or --spectra-only;
  * `--rate-images [K]`: the device also fits every pixel's up-the-ramp samples with a line (wayne_amd/rampfit.py: samples
    behind saturation dropped, jumps above K sigma -- default 5, 0 for none -- cut out of the ramp) and NNNN_rate.fits is
    written beside each _raw file: the raw file's primary header plus RFRN, RFK and RFSAT, then the image HDUs SCI (e-/s),
    ERR, DQ, SAMP and TIME.  The product of a staring visit: a scan's trace is flagged as cosmic rays.  The name is not
    _flt, which is the direct image's here.  Not with --resume, --device-fits or --spectra-only;
  * `--ima [{rate,counts}]`: the device also forms every exposure's calibrated reads (wayne_amd/ima.py: every read with the
    zero read subtracted, linearised, dark-subtracted and in electrons -- per second by default, `counts` for electrons --
    with an error and a data-quality plane) and NNNN_ima.fits is written beside each _raw file, laid out like it: five
    extensions a read, SCI, ERR and DQ with data.  What a scan observer with a reduction of their own differences.  Not
    with --resume, --device-fits or --spectra-only;
  * `--gpus G`: the process starts G rank processes itself (one per GPU of this node, before anything touches a
    GPU) and waits for them; under an external launcher (WORLD_SIZE / RANK set, one process per GPU) it is one
    rank.  Each rank generates its round-robin share of the exposures (observation.py:403-405 is the axis) on the
    CPUs of its GPU's NUMA node.  `--ranks-per-gpu R` starts G x R ranks, R to a GPU (rank r on device r // R):
    on small sub-arrays a visit is bound by one interpreter's lock, not by the GPU.
"""
import argparse
import os
import shutil
import sys

import numpy as np
import yaml

from . import calibration as _cal
from . import detector, grism, ipc, launch, observation, sources, tools, traps
from .trend_generators import scan_speed_varations


class WFC3SimConfigError(Exception):
    pass


def _get(d, key, default=None):
    try:
        v = d[key]
    except (KeyError, TypeError):
        return default
    return v


def ld_table_from_config(target, path=lambda p: p):
    """The optional limb-darkening table of the YAML's `target:` section -> lightcurve.LimbDarkening, or None:
    `ld_table: {law: claret4, wl_um: [...], coeffs: [[...], ...]}` (law optional) or `ld_table_file: FILE`, text with
    columns wl_um and the law's coefficients (`ld_law:` names the law of a file with fewer than five columns); `path`
    resolves FILE like the section's other files.  Every defect is a WFC3SimConfigError."""
    from . import lightcurve
    inline, fname = _get(target, "ld_table"), _get(target, "ld_table_file")
    if inline is None and fname is None:
        if _get(target, "ld_law") is not None:
            raise WFC3SimConfigError("target: ld_law is given without ld_table_file")
        return None
    if inline is not None and fname is not None:
        raise WFC3SimConfigError("target: give ld_table or ld_table_file, not both")
    try:
        if inline is not None:
            if not isinstance(inline, dict):
                raise WFC3SimConfigError("target: ld_table must be a mapping with wl_um, coeffs and an optional law")
            unknown = sorted(set(inline) - {"law", "wl_um", "coeffs"})
            if unknown or "wl_um" not in inline or "coeffs" not in inline:
                raise WFC3SimConfigError("target: ld_table takes wl_um, coeffs and an optional law%s"
                                         % (" (unknown: %s)" % ", ".join(map(str, unknown)) if unknown else ""))
            return lightcurve.LimbDarkening(inline["wl_um"], inline["coeffs"], inline.get("law") or "claret4")
        if not isinstance(fname, str):
            raise WFC3SimConfigError("target: ld_table_file must be a file name")
        return lightcurve.LimbDarkening.from_file(path(fname), _get(target, "ld_law"))
    except (OSError, ValueError) as e:
        raise WFC3SimConfigError("target: limb-darkening table: %s" % e)


def build_observation(cfg, base_dir=".", calibration=None, device=0):
    """YAML dict -> configured Observation (the body of run_visit.run, run_visit.py:41-314)."""
    general, target, obs_cfg = cfg["general"], cfg["target"], cfg["observation"]
    outdir = general["outdir"]
    seed = _get(general, "seed") or 0
    cal = calibration if calibration is not None else _cal.CalibrationSet.synthetic(seed)
    grisms = {"G141": grism.G141, "G102": grism.G102}
    chosen_grism = grisms[obs_cfg["grism"]](cal)
    det = detector.WFC3_IR()

    def path(p):
        return p if os.path.isabs(p) else os.path.join(base_dir, p)

    rebin_resolution = _get(target, "rebin_resolution")
    planet_spectrum_file = _get(target, "planet_spectrum_file")
    transmission = bool(planet_spectrum_file)
    depth_planet = wl_planet = None
    # `ra` / `dec` (degrees, J2000) are an extension of the reference's schema: it reads them off the Open
    # Exoplanet Catalogue entry of `name`; with them the light-curve times become heliocentric (observation.py:340)
    planet = observation.Planet(name=str(_get(target, "name", "planet")),
                                star_temperature=_get(target, "star_temperature", 6100.0),
                                ra_deg=_get(target, "ra", None), dec_deg=_get(target, "dec", None))
    if transmission:
        wl_planet, depth_planet = tools.load_and_sort_spectrum(path(planet_spectrum_file))
        wl_planet, depth_planet = tools.crop_spectrum(0.9, 1.8, wl_planet, depth_planet)      # run_visit.py:152-153
        if rebin_resolution:
            new_wl = tools.wl_at_resolution(rebin_resolution, chosen_grism.wl_limits[0], chosen_grism.wl_limits[1])
            depth_planet = tools.rebin_spec(wl_planet, depth_planet, new_wl)
            wl_planet = new_wl
    stellar_file = _get(target, "stellar_spectrum_file")
    if stellar_file and os.path.exists(path(stellar_file)):
        wl_star, flux_star = tools.load_pheonix_stellar_grid_fits(path(stellar_file))
        if transmission:
            flux_star = tools.rebin_spec(wl_star, flux_star, wl_planet)
        elif rebin_resolution:
            new_wl = tools.wl_at_resolution(rebin_resolution, chosen_grism.wl_limits[0], chosen_grism.wl_limits[1])
            flux_star = tools.rebin_spec(wl_star, flux_star, new_wl)
            wl_star = new_wl
    elif transmission:
        flux_star = tools.blackbody_lambda(wl_planet, planet.star_temperature)                  # run_visit.py:201-203
    else:
        raise WFC3SimConfigError("Must give the stellar spectrum if not using transmission spectroscopy")
    stellar_flux_scaled = flux_star * target["flux_scale"]
    wl = wl_planet if transmission else wl_star

    def maybe_file(v):
        return np.loadtxt(path(v)) if isinstance(v, str) else v

    x_ref, y_ref = maybe_file(obs_cfg["x_ref"]), maybe_file(obs_cfg["y_ref"])
    sky_background = maybe_file(obs_cfg["sky_background"])
    exp_start_times = _get(obs_cfg, "exp_start_times", False)
    if exp_start_times:
        exp_start_times = np.loadtxt(path(exp_start_times))
    spatial_scan = obs_cfg["spatial_scan"]
    sample_rate = obs_cfg["sample_rate"] if spatial_scan else False       # ms
    scan_speed = obs_cfg["scan_speed"] if spatial_scan else False         # px/s
    ssv_type = _get(obs_cfg, "ssv_type")
    ssv_gen = None
    if ssv_type:
        ssv_classes = {"sine": scan_speed_varations.SSVSine, "mod-sine": scan_speed_varations.SSVModulatedSine}
        if ssv_type not in ssv_classes:
            raise WFC3SimConfigError("Invalid ssv_type given")                 # run_visit.py:233-245
        ssv_gen = ssv_classes[ssv_type](*obs_cfg["ssv_coeffs"])

    obs = observation.Observation(outdir if os.path.isabs(outdir) else os.path.join(base_dir, outdir),
                                  calibration=cal, device=device, seed=seed)
    obs.setup_detector(det, obs_cfg["NSAMP"], obs_cfg["SAMPSEQ"], obs_cfg["SUBARRAY"])
    obs.setup_grism(chosen_grism)
    ld_table = ld_table_from_config(target, path)
    if ld_table is not None and not transmission:
        raise WFC3SimConfigError("target: ld_table needs planet_spectrum_file (there is no transit without one)")
    obs.setup_target(planet, wl, depth_planet, stellar_flux_scaled, _get(target, "transit_time"),
                     _get(target, "ldcoeffs"), _get(target, "period"), _get(target, "rp"), _get(target, "sma"),
                     _get(target, "inclination"), _get(target, "eccentricity"), _get(target, "periastron"),
                     _get(target, "stellar_radius"), **({"ld_table": ld_table} if ld_table is not None else {}))
    spot_cfg = _get(target, "spots")
    if spot_cfg is not None:
        if not transmission:
            raise WFC3SimConfigError("target: spots need planet_spectrum_file (there is no transit without one)")
        from . import spots as _spots
        try:
            obs.set_spots(_spots.StarSpots.from_config(spot_cfg, obs.planet_position_at_phase))
        except (TypeError, ValueError) as e:
            raise WFC3SimConfigError("target: spots: %s" % e)
    obs.setup_visit(obs_cfg["start_JD"] or 0.0, obs_cfg["num_orbits"], exp_start_times)
    obs.setup_reductions(obs_cfg["add_dark"], obs_cfg["add_flat"], obs_cfg["add_gain_variations"],
                         obs_cfg["add_non_linear"], obs_cfg["add_initial_bias"])
    obs.setup_observation(x_ref, y_ref, spatial_scan, scan_speed)
    obs.setup_simulator(sample_rate, obs_cfg["clip_values_det_limits"], _get(general, "threads", 2))
    obs.setup_trends(ssv_gen, obs_cfg["x_shifts"], obs_cfg["x_jitter"], obs_cfg["y_shifts"], obs_cfg["y_jitter"])
    obs.setup_noise_sources(sky_background, obs_cfg["cosmic_rate"], obs_cfg["add_read_noise"],
                            obs_cfg["add_stellar_noise"])
    obs.setup_gaussian_noise(obs_cfg["noise_mean"], obs_cfg["noise_std"])
    coeffs = _get(_get(cfg, "trends", {}), "visit_trend_coeffs")
    if coeffs:
        obs.setup_visit_trend(coeffs)
    # optional `contaminants:` section (no reference counterpart): field stars on every exposure; every rank of a
    # --gpus run builds its Observation here, from the same YAML, so each gets the same list
    try:
        contaminants = sources.from_config(_get(cfg, "contaminants"), chosen_grism, wl, stellar_flux_scaled, base_dir)
    except sources.ContaminantConfigError as e:
        raise WFC3SimConfigError(str(e))
    if contaminants:
        obs.setup_contaminants(contaminants)
    # optional `charge_traps:` section (no reference counterpart): per-pixel charge trapping, the ramp effect; absent =
    # none, `{}` = every default
    if isinstance(cfg, dict) and "charge_traps" in cfg:
        try:
            obs.setup_charge_traps(traps.ChargeTraps.from_config(cfg["charge_traps"]))
        except traps.ChargeTrapConfigError as e:
            raise WFC3SimConfigError(str(e))
    # optional `interpixel_capacitance:` section (no reference counterpart): the collected charge coupled into the
    # neighbouring pixels; absent = none, `{}` = the default kernel
    if isinstance(cfg, dict) and "interpixel_capacitance" in cfg:
        try:
            obs.setup_ipc(ipc.InterpixelCapacitance.from_config(cfg["interpixel_capacitance"]))
        except ipc.IpcConfigError as e:
            raise WFC3SimConfigError(str(e))
    return obs


def carried_history(parameter_file):
    """Does the visit's YAML ask for a carried trap history (`charge_traps: {history: carried}`)?  Read before anything
    is started; a file that does not parse says no here and is reported where the visit is built."""
    try:
        with open(parameter_file) as f:
            cfg = yaml.safe_load(f)
    except (OSError, yaml.YAMLError):
        return False
    section = cfg.get("charge_traps") if isinstance(cfg, dict) else None
    return isinstance(section, dict) and section.get("history") == "carried"


def run(argv=None):
    ap = argparse.ArgumentParser(prog="wayne", description=__doc__.split("\n")[0])
    ap.add_argument("-p", "--parameter_file", required=True)
    ap.add_argument("--calibration", default=None, help="directory holding the WFC3 calibration FITS files")
    ap.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    ap.add_argument("--max-exposures", type=int, default=None, help="only the first M exposures")
    ap.add_argument("--gpus", type=int, default=1, help="start rank processes, one per GPU of this node")
    ap.add_argument("--ranks-per-gpu", type=int, default=1, help="... and this many to a GPU (small sub-arrays)")
    ap.add_argument("--dry-run", action="store_true", help=argparse.SUPPRESS)   # ranks meet and report, no GPU work
    ap.add_argument("--resume", action="store_true",
                    help="skip every exposure whose NNNN_raw.fits is already in the output directory, whole and this "
                         "visit's (restart after a failed rank: only the missing files are generated)")
    reads = ap.add_mutually_exclusive_group()
    reads.add_argument("--float64-reads", action="store_true",
                       help="float64 reads from the device (the reference's arithmetic to the file) instead of float32 ones")
    reads.add_argument("--uint16-reads", action="store_true",
                       help="16-bit unsigned reads, the ADC's sample type: the float32 read rounded and saturated to "
                            "0 .. 65535 on the device; the _raw files are then BITPIX 16 / BZERO 32768, a quarter the size")
    ap.add_argument("--device-fits", action="store_true",
                    help="form the data sections of the _raw files on the device and write every file straight from pinned "
                         "memory: the same files, without the host's pass over the samples (not with --spectra-only)")
    ap.add_argument("--expected", choices=("counts", "mean"), default=None,
                    help="render every exposure's noise-free expected image on the device and write it to NNNN_exp.fits "
                         "beside the _raw file: what the electron thrower converges to, given the bin counts the run drew "
                         "(counts) or before the draw (mean); not with --resume, --device-fits, --spectra, --spectra-only")
    ap.add_argument("--rate-images", nargs="?", type=float, const=5.0, default=None, metavar="K",
                    help="fit every pixel's up-the-ramp samples with a line on the device (saturated samples dropped, jumps "
                         "above K sigma cut out; default 5, 0: no jump test) and write rate, error, data quality, samples and "
                         "time to NNNN_rate.fits beside the _raw file; a staring product; not with --resume, --device-fits, "
                         "--spectra-only")
    ap.add_argument("--ima", nargs="?", choices=("rate", "counts"), const="rate", default=None,
                    help="form every exposure's calibrated reads on the device (zero read subtracted, linearised, dark-subtracted, "
                         "in electrons per second, or electrons with `counts`; error and data quality beside them) and write them "
                         "to NNNN_ima.fits beside the _raw file, laid out like it; not with --resume, --device-fits, --spectra-only")
    spectra = ap.add_mutually_exclusive_group()
    spectra.add_argument("--spectra", metavar="OUT.npz", default=None,
                         help="extract every exposure's column spectra on the device and write them to OUT.npz beside "
                              "the _raw files")
    spectra.add_argument("--spectra-only", metavar="OUT.npz", default=None,
                         help="... and write no _raw files: the reads never leave the device")
    ap.add_argument("--reject-cosmics", metavar="K", nargs="?", type=float, const=8.0, default=None,
                    help="with --spectra / --spectra-only: reject cosmic rays on the difference images before the column "
                         "sums, K sigma (default 8) above the largest stencil neighbour; OUT.npz then also holds n_rejected, "
                         "crrej_k and crrej_read_noise")
    ap.add_argument("--channels", metavar="LO:HI:N", default=None,
                    help="with --spectra / --spectra-only: also bin every exposure on the device into N wavelength channels "
                         "of equal width between LO and HI um (flat-fielded at each pixel's wavelength); OUT.npz then also "
                         "holds channels, channel_edges_um, channel_flat, wl_a and wl_b")
    ap.add_argument("--no-channel-flat", action="store_true",
                    help="with --channels: do not divide by the wavelength-dependent flat")
    ap.add_argument("--variances", nargs="?", type=float, const=20.0, default=None, metavar="RN",
                    help="with --spectra / --spectra-only: also deliver the variances of the spectra, the sky levels and "
                         "the channels, RN e- (default 20) the read noise of a difference of two reads; OUT.npz then also "
                         "holds spectra_var, sky_var, channels_var (with --channels) and variance_read_noise")
    ap.add_argument("--optimal", nargs="?", type=int, const=8, default=None, metavar="H",
                    help="with --variances: also deliver the optimal (profile-weighted) spectra and their variances, the "
                         "profile of a column formed over 2H + 1 columns (default 8, 1 .. 16); OUT.npz then also holds "
                         "optimal, optimal_var and optimal_half_width")
    ap.add_argument("--optimal-profile", type=int, default=None, metavar="N",
                    help="with --optimal: a first pass over the first N exposures of each group (window heights and scan "
                         "direction) forms one profile per group on the device, and every exposure is then extracted with "
                         "its group's profile instead of its own; OUT.npz then also holds optimal_profile_exposures")
    ap.add_argument("--optimal-channels", action="store_true",
                    help="with --optimal and --channels: also bin the optimal extraction's weighted pixels into the channels; "
                         "OUT.npz then also holds channels_opt and channels_opt_var (meant for --optimal-profile)")
    args = ap.parse_args(argv)
    ramp_fit = None
    if args.rate_images is not None:
        from . import rampfit as _rampfit
        try:
            ramp_fit = _rampfit.RampFit(k=args.rate_images)
        except ValueError as e:
            raise SystemExit("--rate-images [K] (sigma, finite and >= 0): %s" % e)
    variance = None
    if args.variances is not None:
        if not (args.spectra or args.spectra_only):
            raise SystemExit("--variances needs --spectra or --spectra-only")
        from .extraction import Variances
        try:
            variance = Variances(read_noise=args.variances)
        except ValueError as e:
            raise SystemExit("--variances [RN] (e-, finite and >= 0): %s" % e)
    optimal = None
    if args.optimal is not None:
        if variance is None:
            raise SystemExit("--optimal needs --variances")
        from .extraction import Optimal
        try:
            optimal = Optimal(half_width=args.optimal)
        except ValueError as e:
            raise SystemExit("--optimal [H] (columns, 1 .. 16): %s" % e)
    if args.optimal_channels:
        if optimal is None or args.channels is None:
            raise SystemExit("--optimal-channels needs --optimal and --channels")
        from .extraction import Optimal
        optimal = Optimal(optimal.half_width, channels=True)
    if args.optimal_profile is not None:
        if optimal is None:
            raise SystemExit("--optimal-profile needs --optimal")
        if args.optimal_profile < 1:
            raise SystemExit("--optimal-profile N: at least 1 exposure")
    channels = None
    if args.no_channel_flat and args.channels is None:
        raise SystemExit("--no-channel-flat needs --channels")
    if args.channels is not None:
        if not (args.spectra or args.spectra_only):
            raise SystemExit("--channels needs --spectra or --spectra-only")
        from .extraction import Channels
        try:
            lo, hi, n = args.channels.split(":")
            channels = Channels.linear(float(lo), float(hi), int(n)).with_flat(not args.no_channel_flat)
        except ValueError as e:
            raise SystemExit("--channels LO:HI:N (um, um, 1 .. 256): %s" % e)
    if args.reject_cosmics is not None:
        if not (args.spectra or args.spectra_only):
            raise SystemExit("--reject-cosmics needs --spectra or --spectra-only")
        if not (np.isfinite(args.reject_cosmics) and args.reject_cosmics > 0):
            raise SystemExit("--reject-cosmics: K must be finite and > 0")
    if args.device_fits and args.spectra_only:
        # (the API's refusal, Observation.run_observation's ValueError, raised before any rank process is started)
        raise ValueError("--device-fits forms the data sections of the _raw files; --spectra-only writes none")
    if args.expected:
        # (the API's refusal, Observation.run_observation's ValueError, raised before any rank process is started)
        from . import expected as _expected
        _expected.refuse_combinations(args.expected, resume=args.resume, device_fits=args.device_fits,
                                      spectra=bool(args.spectra), spectra_only=bool(args.spectra_only))
    if ramp_fit is not None:
        # (the API's refusal, Observation.run_observation's ValueError, raised before any rank process is started)
        _rampfit.refuse_combinations(ramp_fit, resume=args.resume, device_fits=args.device_fits,
                                     spectra_only=bool(args.spectra_only))
    if args.ima is not None:
        from . import ima as _ima
        _ima.refuse_combinations(args.ima, resume=args.resume, device_fits=args.device_fits,
                                 spectra_only=bool(args.spectra_only))
    if args.resume and (args.spectra or args.spectra_only):
        raise SystemExit("--spectra / --spectra-only cannot be combined with --resume (a skipped exposure has no spectra)")
    if args.gpus < 1 or args.ranks_per_gpu < 1:
        raise SystemExit("--gpus and --ranks-per-gpu must be at least 1")
    n_ranks = args.gpus * args.ranks_per_gpu
    if (n_ranks > 1 or args.resume or int(os.environ.get("WORLD_SIZE", "1")) > 1) and carried_history(args.parameter_file):
        # a carried trap history chains every exposure to its predecessor on one device: refused here, before any rank
        # process is started
        what = "--gpus > 1" if args.gpus > 1 else "--ranks-per-gpu > 1" if args.ranks_per_gpu > 1 else \
               "--resume" if args.resume else "several ranks (WORLD_SIZE > 1)"
        raise SystemExit("charge_traps history: carried cannot be combined with %s: every exposure starts from the trap "
                         "state its predecessor left on one device" % what)
    given = list(sys.argv[1:] if argv is None else argv)
    if n_ranks > 1 and "WORLD_SIZE" not in os.environ and any(a == "--device" or a.startswith("--device=") for a in given):
        # forwarded to every rank it would put them all on one GPU: each rank takes its device from LOCAL_RANK
        raise SystemExit("--device cannot be combined with --gpus / --ranks-per-gpu (a rank's device is its LOCAL_RANK)")
    if n_ranks > 1 and "WORLD_SIZE" not in os.environ:
        # the launcher: nothing in this process has touched a GPU; the children are ranks of a fresh interpreter each
        child = [a for a in (sys.argv[1:] if argv is None else list(argv))]
        cmd = [sys.executable, "-m", "wayne_amd.run_visit"] + child
        extra = {"PYTHONPATH": os.pathsep.join([os.path.dirname(os.path.dirname(os.path.abspath(__file__)))] +
                                               [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p])}
        codes, _ = launch.launch_ranks(n_ranks, cmd, extra_env=extra)
        if any(codes):
            raise SystemExit("run_visit: rank exit codes %s" % codes)
        print("run_visit: %d ranks done" % n_ranks)
        return None
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    if "WORLD_SIZE" in os.environ and n_ranks not in (1, world_env):
        raise SystemExit("WORLD_SIZE (%d) != --gpus x --ranks-per-gpu (%d)" % (world_env, n_ranks))
    if args.ranks_per_gpu > 1 and "LOCAL_RANK" in os.environ:
        args.device = int(os.environ["LOCAL_RANK"]) // args.ranks_per_gpu
    if os.environ.get("WAYNE_SHARE_GPU") == "1":       # every rank on device 0: a one-GPU box, or several ranks per GPU on small sub-arrays
        args.device = 0
    if args.dry_run:
        # rehearsal of the N-rank path on a box without N GPUs (tests/test_visit_driver.py): every rank parses the
        # visit, takes its round-robin share and says so; nothing touches a GPU
        with open(args.parameter_file) as f:
            cfg = yaml.safe_load(f)
        rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
        n_exp = int(args.max_exposures or 0) or 16
        from . import visit as _visit
        mine = _visit.shard(n_exp, rank, world)
        print("dry-run rank %d/%d device %d threads %s exposures %s" % (
            rank, world, args.device, os.environ.get("OMP_NUM_THREADS", "-"), ",".join(str(i) for i in mine)), flush=True)
        return None
    launch.pin_to_gpu_numa(args.device)
    with open(args.parameter_file) as f:
        cfg = yaml.safe_load(f)
    base_dir = os.path.dirname(os.path.abspath(args.parameter_file))
    cal = _cal.CalibrationSet.from_directory(args.calibration) if args.calibration else None
    obs = build_observation(cfg, base_dir, cal, args.device)
    if args.max_exposures is not None:
        obs.exp_start_times = obs.exp_start_times[:args.max_exposures]
    if args.float64_reads:
        obs.frame_options["out_dtype"] = np.float64
    if args.uint16_reads:
        obs.frame_options["out_dtype"] = np.uint16
    if args.device_fits:
        obs.frame_options["device_fits"] = True
    if args.expected:
        obs.frame_options["expected"] = args.expected
    if ramp_fit is not None:
        obs.frame_options["ramp_fit"] = ramp_fit
    if args.ima is not None:
        obs.frame_options["ima"] = args.ima
    if args.spectra or args.spectra_only:
        obs.frame_options["extraction"] = True
        if args.reject_cosmics is not None:
            from .extraction import CosmicRejection
            obs.frame_options["crrej"] = CosmicRejection(k=args.reject_cosmics)
        if channels is not None:
            obs.frame_options["channels"] = channels
        if variance is not None:
            obs.frame_options["variance"] = variance
        if optimal is not None:
            obs.frame_options["optimal"] = optimal
            obs.optimal_profile_exposures = args.optimal_profile or 0
        obs.spectra_out = args.spectra or args.spectra_only
        obs.spectra_only = bool(args.spectra_only)
    os.makedirs(obs.outdir, exist_ok=True)
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if rank == 0:
        # the visit's own two files are written once, by rank 0 (every rank would write the same bytes, but G x R
        # processes truncating and rewriting one path is a race a reader can see)
        shutil.copy2(args.parameter_file, os.path.join(obs.outdir, os.path.basename(args.parameter_file)))
        t, lc = obs.show_lightcurve()
        np.savetxt(os.path.join(obs.outdir, "visit_plan.txt"), np.column_stack([t, lc]), header="JD white_light_model")
    frames = obs.run_observation(rank=rank, world=world, resume=args.resume)
    print("rank %d/%d: wrote %d files to %s%s" % (rank, world, len(frames), obs.outdir,
                                                 " (%d already there)" % len(obs.skipped) if args.resume else ""))
    return obs


if __name__ == "__main__":
    run()
