#!/usr/bin/env python3
"""Device-side spectral extraction (wayne_exposure_set_extraction, k_extract) against the delivery of reads, side by side
in one process -- GPU only; not part of bench.py.

    python scripts/bench_extract.py [cfg4] [exposures per pass] [repeats] [--out FILE]

Every figure is the median of `repeats` passes with their spread (max - min), the legs taking turns pass by pass so that
a drift of the box falls on all of them.  Resident descriptors in four slots over the context's two streams:
  (a) device_complete          run x n between two synchronisations, no extraction
  (b) device_complete_extract  the same with the default extraction plan set on every slot
  (c) reads_delivered          VisitRunner.run_resident: the reads copied to pinned host memory
  (d) spectra_delivered        VisitRunner.run_resident_spectra: only the spectra block copied, no reads
and the extraction's two kernels by HIP events (wayne_extract_profile), with their algorithmic bytes from the plan
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
    out_path = os.path.join(ROOT, "profiles", "extract.json")
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
        del argv[argv.index("--out"):argv.index("--out") + 2]
    name = argv[0] if len(argv) > 0 else "cfg4"
    n = int(argv[1]) if len(argv) > 1 else 200
    repeats = int(argv[2]) if len(argv) > 2 else 5
    n_host = max(8, n // 4)                                # exposures per pass of the leg that carries reads over PCIe

    cal = calibration.CalibrationSet.synthetic(11)
    det, gr = detector.WFC3_IR(), grism.G141(cal)
    v = synthetic.Visit(name, det, gr, cal, n_exposures=8)
    runner = wvisit.VisitRunner(v, 0)
    eng = runner.engine()
    ctx = eng.ctx
    S, R = v.detector.full_size(v.SUBARRAY), v.NSAMP - 1
    gens = [runner.generator(i) for i in range(4)]
    descs = [g.build_descriptor(eng, out_dtype=runner.out_dtype, rng_mode=runner.rng_mode, extraction=True,
                                **runner.frame_kwargs(i)) for i, g in enumerate(gens)]
    plans = [g.extraction_plan for g in gens]

    def make_resident(extract):
        for slot in range(4):
            ctx.upload(slot, descs[slot])                  # (sets the extraction the descriptor carries)
            if not extract:
                ctx.set_extraction(slot, None)

    def device_complete(count):
        t0 = time.perf_counter()
        for j in range(count):
            ctx.run(j % 4)
        ctx.synchronize()
        return count / (time.perf_counter() - t0)

    legs = ("device_complete", "device_complete_extract", "reads_delivered", "spectra_delivered")
    rate = {leg: [] for leg in legs}
    extract_us = []
    for rep in range(repeats + 1):                         # (the first pass warms up: allocations, pinned buffers, code objects)
        got = {}
        make_resident(False)
        device_complete(8)
        got["device_complete"] = device_complete(n)
        runner.run_resident(8)
        ctx.synchronize()
        t0 = time.perf_counter()
        runner.run_resident(n_host)
        got["reads_delivered"] = n_host / (time.perf_counter() - t0)
        make_resident(True)
        device_complete(8)
        got["device_complete_extract"] = device_complete(n)
        runner.run_resident_spectra(8)
        ctx.synchronize()
        t0 = time.perf_counter()
        runner.run_resident_spectra(n)
        got["spectra_delivered"] = n / (time.perf_counter() - t0)
        # the extraction's kernels alone: HIP events around the pair of launches
        ctx.profile_enable(True)
        ctx.profile_select(["k_extract"])
        ctx.profile_reset()
        for j in range(min(n, 48)):
            ctx.run(j % 4)
        ctx.synchronize()
        p = ctx.extract_profile()
        ctx.profile_enable(False)
        ctx.profile_select(None)
        if rep > 0:
            for leg in legs:
                rate[leg].append(got[leg])
            extract_us.append(p["ms"] / max(p["launches"], 1) * 1e3)

    out = {"config": name, "S": S, "NSAMP": v.NSAMP, "reads_dtype": np.dtype(runner.out_dtype).name,
           "exposures_per_pass": n, "exposures_per_reads_pass": n_host, "repeats": repeats,
           "ramp_variant": ctx.ramp_variant(0)}
    for leg in legs:
        out[leg] = dict(stat(rate[leg], 1), unit="exposures/s")
    med = {leg: out[leg]["median"] for leg in legs}
    out["ratio_b_over_a"] = round(med["device_complete_extract"] / med["device_complete"], 4)
    out["ratio_d_over_b"] = round(med["spectra_delivered"] / med["device_complete_extract"], 4)
    out["ratio_d_over_c"] = round(med["spectra_delivered"] / med["reads_delivered"], 3)
    out["MB_per_exposure"] = {"reads": round((R + 1) * S * S * np.dtype(runner.out_dtype).itemsize / 1e6, 2),
                              "spectra": round((R + 1) * (S + 1) * 8 / 1e6, 4)}
    b = float(np.mean([extraction.algorithmic_bytes(p, S, R, np.dtype(runner.out_dtype).itemsize) for p in plans]))
    us = float(np.median(extract_us))
    out["k_extract"] = {"us": stat(extract_us), "algorithmic_bytes": int(b), "GB_per_s": round(b / (us * 1e-6) / 1e9, 1),
                        "frac_of_8_TB_s": round(b / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                        "row_windows_slot0": plans[0].row_windows.tolist(), "bg_cols": list(plans[0].bg_cols)}
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
