#!/usr/bin/env python3
"""Wavelength-binned channels of the device-side extraction (wayne_exposure_set_channels; k_extract_bins,
k_extract_bins_finish) against the extraction without them, side by side in one process -- GPU only; not part of bench.py.

    python scripts/bench_channels.py [cfg4] [exposures per pass] [repeats] [--out FILE]

Every figure is the median of `repeats` passes with their spread (max - min), the legs taking turns pass by pass so that
a drift of the box falls on all of them.  Resident descriptors in four slots over the context's two streams, for the
extraction alone and with cosmic-ray rejection (k = 8, read noise 20 e-):
  device_complete_extract[_crrej]            run x n between two synchronisations, the default extraction plan
  device_complete_extract_channels[_crrej]   the same with 20 channels between 1.1 and 1.7 um, flat on
  spectra_delivered[_crrej]                  VisitRunner.run_resident_spectra: the spectra block copied to pinned memory
  spectra_delivered_channels[_crrej]         the same: the block carries the channels too
and the extraction's kernels by HIP events (wayne_extract_profile spans all of an exposure's extraction launches; the
two new launches are the difference of the legs with and without channels), with their algorithmic bytes from the plan
(extraction.algorithmic_bytes) and the fraction of 8 TB/s that makes.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wayne_amd import calibration, detector, extraction, grism, synthetic, visit as wvisit  # noqa: E402

HBM_PEAK_GBS = 8000.0


def stat(vals, digits=2):
    return {"median": round(float(np.median(vals)), digits), "spread": round(float(max(vals) - min(vals)), digits),
            "repetitions": [round(float(x), digits) for x in vals]}


def main():
    argv = list(sys.argv[1:])
    out_path = os.path.join(ROOT, "profiles", "channels.json")
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
    crrej = extraction.CosmicRejection()

    def make_resident(reject, binned):
        for slot in range(4):
            ctx.upload(slot, descs[slot])                  # (sets the extraction the descriptor carries, channels too)
            if not binned:
                ctx.set_channels(slot, None)
            if reject:
                ctx.set_crrej(slot, crrej)

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

    tags = [(reject, binned, ("_channels" if binned else "") + ("_crrej" if reject else ""))
            for reject in (False, True) for binned in (False, True)]
    legs = ["device_complete_extract" + t for _, _, t in tags] + ["spectra_delivered" + t for _, _, t in tags]
    rate = {leg: [] for leg in legs}
    us = {"extract" + t: [] for _, _, t in tags}
    sample = None
    for rep in range(repeats + 1):                         # (the first pass warms up: allocations, pinned buffers, code objects)
        got, t = {}, {}
        for reject, binned, tag in tags:
            make_resident(reject, binned)
            device_complete(8)
            got["device_complete_extract" + tag] = device_complete(n)
            runner.run_resident_spectra(8)
            ctx.synchronize()
            t0 = time.perf_counter()
            runner.run_resident_spectra(n)
            got["spectra_delivered" + tag] = n / (time.perf_counter() - t0)
            t["extract" + tag] = kernels_us()
            if binned and not reject:
                ctx.download_spectra(0)
                sample = ctx.channels(0)
        if rep > 0:
            for leg in legs:
                rate[leg].append(got[leg])
            for key in us:
                us[key].append(t[key])

    item = np.dtype(runner.out_dtype).itemsize
    out = {"config": name, "S": S, "NSAMP": v.NSAMP, "reads_dtype": np.dtype(runner.out_dtype).name,
           "exposures_per_pass": n, "repeats": repeats, "ramp_variant": ctx.ramp_variant(0),
           "channels": {"n": channels.n, "lo_um": 1.1, "hi_um": 1.7, "flat": channels.flat},
           "crrej": {"k": crrej.k, "read_noise_e": crrej.read_noise}, "hull_slot0": list(plans[0].hull),
           "channels_last_read_slot0": [round(float(x), 1) for x in sample[R]]}
    for leg in legs:
        out[leg] = dict(stat(rate[leg], 1), unit="exposures/s")
    med = {leg: out[leg]["median"] for leg in legs}
    for suffix in ("", "_crrej"):
        out["ratio_channels_over_extract_device_complete" + suffix] = round(
            med["device_complete_extract_channels" + suffix] / med["device_complete_extract" + suffix], 4)
        out["ratio_channels_over_extract_delivered" + suffix] = round(
            med["spectra_delivered_channels" + suffix] / med["spectra_delivered" + suffix], 4)
    for reject, binned, tag in tags:
        b = float(np.mean([extraction.algorithmic_bytes(p, S, R, item, crrej=reject, channels=binned) for p in plans]))
        t_us = float(np.median(us["extract" + tag]))
        out["k_extract" + tag] = {"us": stat(us["extract" + tag]), "algorithmic_bytes": int(b),
                                  "GB_per_s": round(b / (t_us * 1e-6) / 1e9, 1),
                                  "frac_of_8_TB_s": round(b / (t_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)}
    for suffix in ("", "_crrej"):
        with_, without = out["k_extract_channels" + suffix], out["k_extract" + suffix]
        t_us = with_["us"]["median"] - without["us"]["median"]
        b = with_["algorithmic_bytes"] - without["algorithmic_bytes"]
        out["k_extract_bins" + suffix] = {"kernels": "k_extract_bins<T, %s> + k_extract_bins_finish" % ("true" if suffix else "false"),
                                          "us_by_difference": round(t_us, 2), "algorithmic_bytes": int(b),
                                          "bytes_over_extraction": round(b / without["algorithmic_bytes"], 4),
                                          "frac_of_8_TB_s": round(b / (t_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)}
    out["row_windows_slot0"] = plans[0].row_windows.tolist()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
