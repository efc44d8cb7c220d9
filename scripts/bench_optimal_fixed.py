#!/usr/bin/env python3
"""The optimal extraction with a supplied profile (wayne_exposure_set_optimal_profile; k_extract_optimal_fixed) and the
delivery of the profile planes (wayne_exposure_deliver_profile; k_extract_profile) against the optimal extraction with the
exposure's own profile, side by side in one process -- GPU only; not part of bench.py.

    python scripts/bench_optimal_fixed.py [cfg4] [exposures per pass] [repeats] [--out FILE]

The pattern of scripts/bench_optimal.py: every figure is the median of `repeats` passes with their spread (max - min), the
legs taking turns pass by pass; resident descriptors in four slots over the context's two streams; variances (read noise 20
e-) and the optimal extraction (half width 8) in every leg, without or with cosmic-ray rejection:
  ..._opt           the exposure's own profile (k_extract_optimal: what the parent commit launches)
  ..._opt_fixed     a supplied profile (each slot's own planes, normalised by extraction.ProfileSum)
  ..._opt_deliver   the own profile, and the planes written beside it (never copied here: a visit fetches a handful)
  ..._chan_opt / _chan_opt_fixed            20 channels over 1.1 - 1.7 um beside the optimal extraction (own / supplied profile)
  ..._chan_opt_cho / _chan_opt_fixed_cho    the same with the optimal channels (channels_opt, channels_opt_var)
device_complete_extract*: run x n between two synchronisations; spectra_delivered*: VisitRunner.run_resident_spectra; and the
extraction's kernels by HIP events (wayne_extract_profile spans all of an exposure's extraction launches), with their
algorithmic bytes from the plan and those as a share of 8 TB/s.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wayne_amd import calibration, detector, extraction, grism, synthetic, visit as wvisit  # noqa: E402

HBM_BYTES_PER_S = 8e12


def stat(vals, digits=2):
    return {"median": round(float(np.median(vals)), digits), "spread": round(float(max(vals) - min(vals)), digits),
            "repetitions": [round(float(x), digits) for x in vals]}


def main():
    argv = list(sys.argv[1:])
    out_path = os.path.join(ROOT, "profiles", "optimal_fixed.json")
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
        del argv[argv.index("--out"):argv.index("--out") + 2]
    name = argv[0] if len(argv) > 0 else "cfg4"
    n = int(argv[1]) if len(argv) > 1 else 200
    repeats = int(argv[2]) if len(argv) > 2 else 5

    cal = calibration.CalibrationSet.synthetic(11)
    det, gr = detector.WFC3_IR(), grism.G141(cal)
    v = synthetic.Visit(name, det, gr, cal, n_exposures=8)
    runner = wvisit.VisitRunner(v, 0)
    eng = runner.engine()
    ctx = eng.ctx
    S, R = v.detector.full_size(v.SUBARRAY), v.NSAMP - 1
    crrej, variance, optimal = extraction.CosmicRejection(), extraction.Variances(), extraction.Optimal()
    gens = [runner.generator(i) for i in range(4)]
    descs = [g.build_descriptor(eng, out_dtype=runner.out_dtype, rng_mode=runner.rng_mode,
                                extraction=extraction.ExtractionOptions(variance=variance, optimal=optimal),
                                **runner.frame_kwargs(i))
             for i, g in enumerate(gens)]
    plans = [g.extraction_plan for g in gens]
    channels = extraction.Channels.linear(1.1, 1.7, 20)
    gens_ch = [runner.generator(i) for i in range(4)]
    descs_ch = [g.build_descriptor(eng, out_dtype=runner.out_dtype, rng_mode=runner.rng_mode,
                                   extraction=extraction.ExtractionOptions(channels=channels, variance=variance, optimal=optimal),
                                   **runner.frame_kwargs(i))
                for i, g in enumerate(gens_ch)]
    plans_ch = [g.extraction_plan for g in gens_ch]

    # each slot's profile: its own planes, normalised
    profiles = []
    for slot in range(4):
        ctx.upload(slot, descs[slot])
        ctx.deliver_profile(slot)
        ctx.run(slot)
        ctx.download_spectra(slot)
        profiles.append(extraction.ProfileSum().add(plans[slot], ctx.profile_planes(slot)).profile())

    def make_resident(reject, mode):
        for slot in range(4):
            ctx.upload(slot, (descs_ch if mode.startswith("chan") else descs)[slot])   # (sets the extraction the descriptor carries)
            if reject:
                ctx.set_crrej(slot, crrej)
            if "fixed" in mode:
                ctx.set_optimal_profile(slot, profiles[slot])
            if mode == "deliver":
                ctx.deliver_profile(slot)
            if mode.endswith("cho"):
                ctx.set_optimal_channels(slot)

    def device_complete(count):
        t0 = time.perf_counter()
        for j in range(count):
            ctx.run(j % 4)
        ctx.synchronize()
        return count / (time.perf_counter() - t0)

    def kernels_us():
        ctx.profile_enable(True)
        ctx.profile_select(["k_extract"])
        ctx.profile_reset()
        for j in range(min(n, 48)):
            ctx.run(j % 4)
        ctx.synchronize()
        p = ctx.extract_profile()
        ctx.profile_enable(False)
        ctx.profile_select(None)
        return p["ms"] / max(p["launches"], 1) * 1e3

    def tag_of(reject, mode):
        chan = mode.startswith("chan")
        rest = mode[4:].strip("_") if chan else mode
        return "_var" + ("_crrej" if reject else "") + ("_chan" if chan else "") + "_opt" + ("_" + rest if rest else "")

    MODES = ("", "fixed", "deliver", "chan", "chan_cho", "chan_fixed", "chan_fixed_cho")
    tags = [(reject, mode, tag_of(reject, mode)) for reject in (False, True) for mode in MODES]
    legs = ["device_complete_extract" + t[2] for t in tags] + ["spectra_delivered" + t[2] for t in tags]
    rate = {leg: [] for leg in legs}
    us = {"extract" + t[2]: [] for t in tags}
    sample = {}
    for rep in range(repeats + 1):                         # (the first pass warms up: allocations, pinned buffers, code objects)
        got, t = {}, {}
        for reject, mode, tag in tags:
            make_resident(reject, mode)
            device_complete(8)
            got["device_complete_extract" + tag] = device_complete(n)
            runner.run_resident_spectra(8)
            ctx.synchronize()
            t0 = time.perf_counter()
            runner.run_resident_spectra(n)
            got["spectra_delivered" + tag] = n / (time.perf_counter() - t0)
            t["extract" + tag] = kernels_us()
            if not reject and mode in ("", "fixed"):
                spectra, _ = ctx.download_spectra(0)
                sample[mode] = (spectra,) + ctx.optimal(0)
        if rep > 0:
            for leg in legs:
                rate[leg].append(got[leg])
            for key in us:
                us[key].append(t[key])

    item = np.dtype(runner.out_dtype).itemsize
    spectra, own_flux, own_var = sample[""]
    _, fix_flux, fix_var = sample["fixed"]
    both = (own_flux[R] != spectra[R]) & (fix_flux[R] != spectra[R])
    out = {"config": name, "S": S, "NSAMP": v.NSAMP, "reads_dtype": np.dtype(runner.out_dtype).name,
           "exposures_per_pass": n, "repeats": repeats, "ramp_variant": ctx.ramp_variant(0),
           "crrej": {"k": crrej.k, "read_noise_e": crrej.read_noise}, "variance": {"read_noise_e": variance.read_noise},
           "optimal": {"half_width": optimal.half_width},
           "profile_doubles_slot0": int(profiles[0].planes.size),
           "last_read_slot0": {"columns_optimal_in_both": int(both.sum()),
                               "median_fixed_var_over_own_var": round(float(np.median(fix_var[R][both] / own_var[R][both])), 4)
                               if both.any() else None,
                               "max_rel_flux_difference": float(np.abs(fix_flux[R][both] / own_flux[R][both] - 1.0).max())
                               if both.any() else None}}
    for leg in legs:
        out[leg] = dict(stat(rate[leg], 1), unit="exposures/s")
    med = {leg: out[leg]["median"] for leg in legs}
    for reject, mode, tag in tags:
        if mode in ("fixed", "deliver"):
            base = "_var" + ("_crrej" if reject else "") + "_opt"
            out["ratio_%s_over_own_device_complete%s" % (mode, "_crrej" if reject else "")] = round(
                med["device_complete_extract" + tag] / med["device_complete_extract" + base], 4)
            out["ratio_%s_over_own_delivered%s" % (mode, "_crrej" if reject else "")] = round(
                med["spectra_delivered" + tag] / med["spectra_delivered" + base], 4)
    for reject, mode, tag in tags:
        chan = mode.startswith("chan")
        b = float(np.mean([extraction.algorithmic_bytes(p, S, R, item, crrej=reject, channels=chan, variance=True, optimal=True,
                                                        profile="fixed" in mode, deliver_profile=mode == "deliver",
                                                        optimal_channels=mode.endswith("cho")) for p in (plans_ch if chan else plans)]))
        t_us = float(np.median(us["extract" + tag]))
        out["k_extract" + tag] = {"us": stat(us["extract" + tag]), "algorithmic_bytes": int(b),
                                  "GB_per_s": round(b / (t_us * 1e-6) / 1e9, 1),
                                  "share_of_8_TB_per_s": round(b / (t_us * 1e-6) / HBM_BYTES_PER_S, 4)}
    for reject, mode, tag in tags:
        if mode.endswith("cho"):                           # the optimal channels against the same leg without them
            base_tag = tag_of(reject, mode[:-4])
            out["optimal_channels_cost" + tag] = {
                "us_by_difference": round(out["k_extract" + tag]["us"]["median"] - out["k_extract" + base_tag]["us"]["median"], 2),
                "algorithmic_bytes": out["k_extract" + tag]["algorithmic_bytes"] - out["k_extract" + base_tag]["algorithmic_bytes"],
                "ratio_device_complete": round(med["device_complete_extract" + tag] / med["device_complete_extract" + base_tag], 4),
                "ratio_delivered": round(med["spectra_delivered" + tag] / med["spectra_delivered" + base_tag], 4)}
    for reject, mode, tag in tags:
        if mode in ("fixed", "deliver"):
            base = out["k_extract_var" + ("_crrej" if reject else "") + "_opt"]
            out["%s_minus_own%s" % (mode, "_crrej" if reject else "")] = {
                "us_by_difference": round(out["k_extract" + tag]["us"]["median"] - base["us"]["median"], 2),
                "algorithmic_bytes": out["k_extract" + tag]["algorithmic_bytes"] - base["algorithmic_bytes"]}
    out["row_windows_slot0"] = plans[0].row_windows.tolist()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
