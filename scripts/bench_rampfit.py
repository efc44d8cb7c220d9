#!/usr/bin/env python3
"""The cost of the ramp fit (k_ramp_fit) beside an exposure, on the metric's configuration: the kernel's HIP-event time
against the bytes it has to move (R + 1 reads, R dark values, four linearity coefficients and the pixel flat in, 20 bytes
out, per light-sensitive pixel), and device-complete exposures per second with and without the option over four resident
slots on the context's two streams.  Medians of `repeats` passes behind a warm-up pass.  GPU only.  No test asserts any
of it.

    python scripts/bench_rampfit.py [config=cfg4] [exposures per pass=200] [repeats=5] [--out profiles/rampfit.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wayne_amd import _lib, calibration, detector, grism, synthetic, visit as wvisit  # noqa: E402

HBM_BYTES_PER_S = 8e12


def stat(vals, digits=2):
    return {"median": round(float(np.median(vals)), digits), "spread": round(float(max(vals) - min(vals)), digits),
            "repetitions": [round(float(x), digits) for x in vals]}


def main():
    argv = list(sys.argv[1:])
    out_path = os.path.join(ROOT, "profiles", "rampfit.json")
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
    item = np.dtype(runner.out_dtype).itemsize
    descs = [runner.generator(i).build_descriptor(eng, out_dtype=runner.out_dtype, rng_mode=runner.rng_mode, ramp_fit=True,
                                                  **runner.frame_kwargs(i)) for i in range(4)]

    def make_resident(fit):
        for slot in range(4):
            ctx.upload(slot, descs[slot])                  # (sets the ramp fit the descriptor carries)
            if not fit:
                ctx.set_rampfit(slot, None)

    def device_complete(count):
        t0 = time.perf_counter()
        for j in range(count):
            ctx.run(j % 4)
        ctx.synchronize()
        return count / (time.perf_counter() - t0)

    legs = ("device_complete", "device_complete_rampfit")
    rate = {leg: [] for leg in legs}
    kernel_us = []
    flagged = cut = None
    for rep in range(repeats + 1):                         # (the first pass warms up: allocations, code objects)
        got = {}
        make_resident(False)
        device_complete(8)
        got["device_complete"] = device_complete(n)
        make_resident(True)
        device_complete(8)
        got["device_complete_rampfit"] = device_complete(n)
        # the kernel alone: HIP events around its launch
        ctx.profile_enable(True)
        ctx.profile_select(["k_ramp_fit"])
        ctx.profile_reset()
        for j in range(min(n, 48)):
            ctx.run(j % 4)
        ctx.synchronize()
        p = ctx.rampfit_profile()
        ctx.profile_enable(False)
        ctx.profile_select(None)
        if rep > 0:
            for leg in legs:
                rate[leg].append(got[leg])
            kernel_us.append(p["ms"] / max(p["launches"], 1) * 1e3)
        else:
            _, _, word = ctx.rampfit(0)
            inner = word[5:-5, 5:-5]
            flagged, cut = int(((inner & 0xFFFF) != 0).sum()), int(((inner >> 16) < R).sum())

    N = S - 10
    bytes_in = N * N * ((R + 1) * item + R * 4 + 4 * 4 + 4)
    bytes_out = S * S * 20
    us = float(np.median(kernel_us))
    out = {"config": name, "S": S, "NSAMP": v.NSAMP, "reads_dtype": np.dtype(runner.out_dtype).name,
           "exposures_per_pass": n, "repeats": repeats, "ramp_variant": ctx.ramp_variant(0),
           "library": _lib.library_info()[0].replace(ROOT + os.sep, ""),
           "k_ramp_fit_us": stat(kernel_us, 1),
           "bytes_moved": {"in": bytes_in, "out": bytes_out, "total": bytes_in + bytes_out,
                           "us_at_8_TB_per_s": round((bytes_in + bytes_out) / HBM_BYTES_PER_S * 1e6, 1),
                           "achieved_TB_per_s": round((bytes_in + bytes_out) / (us * 1e-6) / 1e12, 3) if us > 0 else None},
           "scan_pixels_flagged_as_jumps": flagged, "pixels_cut_by_saturation": cut}
    for leg in legs:
        out[leg] = dict(stat(rate[leg], 1), unit="exposures/s")
    out["ratio_rampfit_over_none"] = round(out["device_complete_rampfit"]["median"] / out["device_complete"]["median"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
    print("wrote", out_path)


if __name__ == "__main__":
    main()
