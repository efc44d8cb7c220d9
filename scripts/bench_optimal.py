#!/usr/bin/env python3
"""The optimal (profile-weighted) extraction (wayne_exposure_set_optimal; k_extract_optimal and k_extract_optimal_finish)
against the extraction with variances alone, side by side in one process -- GPU only; not part of bench.py.

    python scripts/bench_optimal.py [cfg4] [exposures per pass] [repeats] [--out FILE]

Every figure is the median of `repeats` passes with their spread (max - min), the legs taking turns pass by pass so that
a drift of the box falls on all of them.  Resident descriptors in four slots over the context's two streams; a leg is the
extraction with variances (read noise 20 e-), without or with cosmic-ray rejection (k = 8, read noise 20 e-), and each of
those without and with the optimal extraction (half width 8):
  device_complete_extract_var[_crrej][_opt]   run x n between two synchronisations, the default extraction plan
  spectra_delivered_var[_crrej][_opt]         VisitRunner.run_resident_spectra: the spectra block copied to pinned memory
                                              (with optimal and optimal_var it is about half as long again)
and the extraction's kernels by HIP events (wayne_extract_profile spans all of an exposure's extraction launches, so the
two optimal kernels' time is the difference of a leg with and without them), with their algorithmic bytes from the plan
(extraction.algorithmic_bytes) and those as a share of 8 TB/s.
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
    out_path = os.path.join(ROOT, "profiles", "optimal.json")
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
                                extraction=extraction.ExtractionOptions(variance=variance), **runner.frame_kwargs(i))
             for i, g in enumerate(gens)]
    plans = [g.extraction_plan for g in gens]

    def make_resident(reject, opt):
        for slot in range(4):
            ctx.upload(slot, descs[slot])                  # (sets the extraction the descriptor carries, variances too)
            if reject:
                ctx.set_crrej(slot, crrej)
            if opt:
                ctx.set_optimal(slot, optimal)

    def device_complete(count):
        t0 = time.perf_counter()
        for j in range(count):
            ctx.run(j % 4)
        ctx.synchronize()
        return count / (time.perf_counter() - t0)

    def kernels_us():
        """the extraction's kernels alone: HIP events around the launches of one exposure"""
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

    tags = [(reject, opt, "_var" + ("_crrej" if reject else "") + ("_opt" if opt else ""))
            for reject in (False, True) for opt in (False, True)]
    legs = ["device_complete_extract" + t[2] for t in tags] + ["spectra_delivered" + t[2] for t in tags]
    rate = {leg: [] for leg in legs}
    us = {"extract" + t[2]: [] for t in tags}
    sample = None
    for rep in range(repeats + 1):                         # (the first pass warms up: allocations, pinned buffers, code objects)
        got, t = {}, {}
        for reject, opt, tag in tags:
            make_resident(reject, opt)
            device_complete(8)
            got["device_complete_extract" + tag] = device_complete(n)
            runner.run_resident_spectra(8)
            ctx.synchronize()
            t0 = time.perf_counter()
            runner.run_resident_spectra(n)
            got["spectra_delivered" + tag] = n / (time.perf_counter() - t0)
            t["extract" + tag] = kernels_us()
            if opt and not reject:
                spectra, _ = ctx.download_spectra(0)
                sample = (spectra, ctx.variances(0)[0]) + ctx.optimal(0)
        if rep > 0:
            for leg in legs:
                rate[leg].append(got[leg])
            for key in us:
                us[key].append(t[key])

    item = np.dtype(runner.out_dtype).itemsize
    spectra, spectra_var, opt_flux, opt_var = sample
    differs = opt_flux[R] != spectra[R]                    # the columns of the last-read product that took the optimal branch
    out = {"config": name, "S": S, "NSAMP": v.NSAMP, "reads_dtype": np.dtype(runner.out_dtype).name,
           "exposures_per_pass": n, "repeats": repeats, "ramp_variant": ctx.ramp_variant(0),
           "crrej": {"k": crrej.k, "read_noise_e": crrej.read_noise}, "variance": {"read_noise_e": variance.read_noise},
           "optimal": {"half_width": optimal.half_width},
           "last_read_slot0": {"optimal_columns": int(differs.sum()), "fallback_columns": int((~differs).sum()),
                               "median_optimal_var_over_spectra_var": round(float(np.median(opt_var[R][differs] / spectra_var[R][differs])), 4)
                               if differs.any() else None}}
    for leg in legs:
        out[leg] = dict(stat(rate[leg], 1), unit="exposures/s")
    med = {leg: out[leg]["median"] for leg in legs}
    for reject, opt, tag in tags:
        if not opt:
            out["ratio_opt_over_none_device_complete" + tag] = round(
                med["device_complete_extract" + tag + "_opt"] / med["device_complete_extract" + tag], 4)
            out["ratio_opt_over_none_delivered" + tag] = round(
                med["spectra_delivered" + tag + "_opt"] / med["spectra_delivered" + tag], 4)
    for reject, opt, tag in tags:
        b = float(np.mean([extraction.algorithmic_bytes(p, S, R, item, crrej=reject, variance=True, optimal=opt) for p in plans]))
        t_us = float(np.median(us["extract" + tag]))
        out["k_extract" + tag] = {"us": stat(us["extract" + tag]), "algorithmic_bytes": int(b),
                                  "GB_per_s": round(b / (t_us * 1e-6) / 1e9, 1),
                                  "share_of_8_TB_per_s": round(b / (t_us * 1e-6) / HBM_BYTES_PER_S, 4)}
    for reject, opt, tag in tags:
        if not opt:
            with_, without = out["k_extract" + tag + "_opt"], out["k_extract" + tag]
            d_us = with_["us"]["median"] - without["us"]["median"]
            d_b = with_["algorithmic_bytes"] - without["algorithmic_bytes"]
            out["optimal_cost" + tag] = {"us_by_difference": round(d_us, 2), "algorithmic_bytes": d_b,
                                         "bytes_over_extraction": round(with_["algorithmic_bytes"] / without["algorithmic_bytes"] - 1.0, 4),
                                         "GB_per_s": round(d_b / (d_us * 1e-6) / 1e9, 1) if d_us > 0 else None,
                                         "share_of_8_TB_per_s": round(d_b / (d_us * 1e-6) / HBM_BYTES_PER_S, 4) if d_us > 0 else None}
    out["row_windows_slot0"] = plans[0].row_windows.tolist()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
