#!/usr/bin/env python3
"""Variances of the device-side extraction (wayne_exposure_set_variance; the VAR instantiations of k_extract_rows,
k_extract_finish, k_extract_bins and k_extract_bins_finish) against the extraction without them, side by side in one
process -- GPU only; not part of bench.py.

    python scripts/bench_variance.py [cfg4] [exposures per pass] [repeats] [--out FILE]

Every figure is the median of `repeats` passes with their spread (max - min), the legs taking turns pass by pass so that
a drift of the box falls on all of them.  Resident descriptors in four slots over the context's two streams; a leg is the
extraction alone or with 20 channels between 1.1 and 1.7 um (flat on), without or with cosmic-ray rejection (k = 8, read
noise 20 e-), and each of those without and with variances (read noise 20 e-):
  device_complete_extract[_channels][_crrej][_var]   run x n between two synchronisations, the default extraction plan
  spectra_delivered[_channels][_crrej][_var]         VisitRunner.run_resident_spectra: the spectra block copied to pinned
                                                     memory (with variances it is about twice as long)
and the extraction's kernels by HIP events (wayne_extract_profile spans all of an exposure's extraction launches; the
variances launch nothing of their own, so their time is the difference of a leg with and without them), with their
algorithmic bytes from the plan (extraction.algorithmic_bytes).
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wayne_amd import calibration, detector, extraction, grism, synthetic, visit as wvisit  # noqa: E402


def stat(vals, digits=2):
    return {"median": round(float(np.median(vals)), digits), "spread": round(float(max(vals) - min(vals)), digits),
            "repetitions": [round(float(x), digits) for x in vals]}


def main():
    argv = list(sys.argv[1:])
    out_path = os.path.join(ROOT, "profiles", "variance.json")
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
    channels = extraction.Channels.linear(1.1, 1.7, 20)
    gens = [runner.generator(i) for i in range(4)]
    descs = [g.build_descriptor(eng, out_dtype=runner.out_dtype, rng_mode=runner.rng_mode,
                                extraction=extraction.ExtractionOptions(channels=channels), **runner.frame_kwargs(i))
             for i, g in enumerate(gens)]
    plans = [g.extraction_plan for g in gens]
    crrej, variance = extraction.CosmicRejection(), extraction.Variances()

    def make_resident(reject, binned, var):
        for slot in range(4):
            ctx.upload(slot, descs[slot])                  # (sets the extraction the descriptor carries, channels too)
            if not binned:
                ctx.set_channels(slot, None)
            if reject:
                ctx.set_crrej(slot, crrej)
            if var:
                ctx.set_variance(slot, variance)

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

    tags = [(reject, binned, var, ("_channels" if binned else "") + ("_crrej" if reject else "") + ("_var" if var else ""))
            for reject in (False, True) for binned in (False, True) for var in (False, True)]
    legs = ["device_complete_extract" + t[3] for t in tags] + ["spectra_delivered" + t[3] for t in tags]
    rate = {leg: [] for leg in legs}
    us = {"extract" + t[3]: [] for t in tags}
    sample = None
    for rep in range(repeats + 1):                         # (the first pass warms up: allocations, pinned buffers, code objects)
        got, t = {}, {}
        for reject, binned, var, tag in tags:
            make_resident(reject, binned, var)
            device_complete(8)
            got["device_complete_extract" + tag] = device_complete(n)
            runner.run_resident_spectra(8)
            ctx.synchronize()
            t0 = time.perf_counter()
            runner.run_resident_spectra(n)
            got["spectra_delivered" + tag] = n / (time.perf_counter() - t0)
            t["extract" + tag] = kernels_us()
            if binned and var and not reject:
                ctx.download_spectra(0)
                sample = ctx.variances(0)
        if rep > 0:
            for leg in legs:
                rate[leg].append(got[leg])
            for key in us:
                us[key].append(t[key])

    item = np.dtype(runner.out_dtype).itemsize
    out = {"config": name, "S": S, "NSAMP": v.NSAMP, "reads_dtype": np.dtype(runner.out_dtype).name,
           "exposures_per_pass": n, "repeats": repeats, "ramp_variant": ctx.ramp_variant(0),
           "channels": {"n": channels.n, "lo_um": 1.1, "hi_um": 1.7, "flat": channels.flat},
           "crrej": {"k": crrej.k, "read_noise_e": crrej.read_noise}, "variance": {"read_noise_e": variance.read_noise},
           "hull_slot0": list(plans[0].hull),
           "channels_sigma_last_read_slot0": [round(float(x), 1) for x in np.sqrt(sample[2][R])]}
    for leg in legs:
        out[leg] = dict(stat(rate[leg], 1), unit="exposures/s")
    med = {leg: out[leg]["median"] for leg in legs}
    for reject, binned, var, tag in tags:
        if not var:
            out["ratio_var_over_none_device_complete" + tag] = round(
                med["device_complete_extract" + tag + "_var"] / med["device_complete_extract" + tag], 4)
            out["ratio_var_over_none_delivered" + tag] = round(
                med["spectra_delivered" + tag + "_var"] / med["spectra_delivered" + tag], 4)
    for reject, binned, var, tag in tags:
        b = float(np.mean([extraction.algorithmic_bytes(p, S, R, item, crrej=reject, channels=binned, variance=var) for p in plans]))
        t_us = float(np.median(us["extract" + tag]))
        out["k_extract" + tag] = {"us": stat(us["extract" + tag]), "algorithmic_bytes": int(b),
                                  "GB_per_s": round(b / (t_us * 1e-6) / 1e9, 1)}
    for reject, binned, var, tag in tags:
        if not var:
            with_, without = out["k_extract" + tag + "_var"], out["k_extract" + tag]
            out["variance_cost" + tag] = {"us_by_difference": round(with_["us"]["median"] - without["us"]["median"], 2),
                                          "algorithmic_bytes": with_["algorithmic_bytes"] - without["algorithmic_bytes"],
                                          "bytes_over_extraction": round(with_["algorithmic_bytes"] / without["algorithmic_bytes"] - 1.0, 4)}
    out["row_windows_slot0"] = plans[0].row_windows.tolist()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
