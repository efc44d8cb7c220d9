#!/usr/bin/env python3
"""The cost of the calibrated reads (k_ima) beside an exposure, on the metric's configuration: the kernel's HIP-event time
against the bytes it has to move (R + 1 reads, R dark values, four linearity coefficients and the pixel flat in; the
payload, padding included, out), for float32 and uint16 reads and both units, set beside k_fits_words's share of the copy
ceiling (profiles/device_fits.json); and device-complete exposures per second with and without the option over four
resident slots on the context's two streams.  Medians of `repeats` passes behind a warm-up pass.  GPU only.  No test
asserts any of it.

    python scripts/bench_ima.py [config=cfg4] [exposures per pass=200] [repeats=5] [--out profiles/ima.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wayne_amd import _lib, calibration, detector, grism, ima, synthetic, visit as wvisit  # noqa: E402

HBM_BYTES_PER_S = 8e12


def stat(vals, digits=2):
    return {"median": round(float(np.median(vals)), digits), "spread": round(float(max(vals) - min(vals)), digits),
            "repetitions": [round(float(x), digits) for x in vals]}


def copy_ceiling():
    """(bytes/s of the copy ceiling, k_fits_words's fractions of it) as profiles/device_fits.json recorded them."""
    try:
        with open(os.path.join(ROOT, "profiles", "device_fits.json")) as f:
            parts = json.load(f)["parts"]
        k = parts["float32"]["k_fits_words"]
        return k["bytes_per_s"] / k["fraction_of_copy_ceiling"], {d: parts[d]["k_fits_words"]["fraction_of_copy_ceiling"] for d in parts}
    except (OSError, KeyError, ValueError):
        return None, {}


def main():
    argv = list(sys.argv[1:])
    out_path = os.path.join(ROOT, "profiles", "ima.json")
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
        del argv[argv.index("--out"):argv.index("--out") + 2]
    name = argv[0] if len(argv) > 0 else "cfg4"
    n = int(argv[1]) if len(argv) > 1 else 200
    repeats = int(argv[2]) if len(argv) > 2 else 5

    cal = calibration.CalibrationSet.synthetic(11)
    det, gr = detector.WFC3_IR(), grism.G141(cal)
    v = synthetic.Visit(name, det, gr, cal, n_exposures=8)
    S, R = v.detector.full_size(v.SUBARRAY), v.NSAMP - 1
    lay = ima.layout(S, R)
    ceiling, fits_share = copy_ceiling()
    out = {"config": name, "S": S, "NSAMP": v.NSAMP, "exposures_per_pass": n, "repeats": repeats,
           "library": _lib.library_info()[0].replace(ROOT + os.sep, ""), "payload_bytes": lay.nbytes,
           "copy_ceiling_bytes_per_s": ceiling, "k_fits_words_fraction_of_copy_ceiling": fits_share, "reads": {}}

    for dtype in (np.float32, np.uint16):
        runner = wvisit.VisitRunner(v, 0, out_dtype=dtype)
        eng = runner.engine()
        ctx = eng.ctx
        item = np.dtype(dtype).itemsize
        descs = [runner.generator(i).build_descriptor(eng, out_dtype=dtype, rng_mode=runner.rng_mode, **runner.frame_kwargs(i))
                 for i in range(4)]

        def make_resident(opt):
            for slot in range(4):
                ctx.upload(slot, descs[slot])
                if opt:
                    ctx.set_ima(slot, opt)

        def device_complete(count):
            t0 = time.perf_counter()
            for j in range(count):
                ctx.run(j % 4)
            ctx.synchronize()
            return count / (time.perf_counter() - t0)

        legs = ("device_complete", "device_complete_ima")
        rate = {leg: [] for leg in legs}
        kernel_us = {"rate": [], "counts": []}
        for rep in range(repeats + 1):                         # (the first pass warms up: allocations, code objects)
            got = {}
            make_resident(None)
            device_complete(8)
            got["device_complete"] = device_complete(n)
            us = {}
            for units in ("counts", "rate"):
                make_resident(units)
                device_complete(8)
                if units == "rate":
                    got["device_complete_ima"] = device_complete(n)
                # the kernel alone: HIP events around its launch
                ctx.profile_enable(True)
                ctx.profile_select(["k_ima"])
                ctx.profile_reset()
                for j in range(min(n, 48)):
                    ctx.run(j % 4)
                ctx.synchronize()
                p = ctx.ima_profile()
                ctx.profile_enable(False)
                ctx.profile_select(None)
                us[units] = p["ms"] / max(p["launches"], 1) * 1e3
            if rep > 0:
                for leg in legs:
                    rate[leg].append(got[leg])
                for units in us:
                    kernel_us[units].append(us[units])

        bytes_in = S * S * ((R + 1) * item + R * 4 + 4 * 4 + 4)
        bytes_out = lay.nbytes
        part = {"ramp_variant": ctx.ramp_variant(0),
                "bytes_moved": {"in": bytes_in, "out": bytes_out, "total": bytes_in + bytes_out,
                                "us_at_8_TB_per_s": round((bytes_in + bytes_out) / HBM_BYTES_PER_S * 1e6, 1)}}
        for units in ("rate", "counts"):
            us = float(np.median(kernel_us[units]))
            bps = (bytes_in + bytes_out) / (us * 1e-6) if us > 0 else None
            part["k_ima_us_" + units] = stat(kernel_us[units], 1)
            part["bytes_per_s_" + units] = bps
            part["fraction_of_copy_ceiling_" + units] = round(bps / ceiling, 4) if bps and ceiling else None
        for leg in legs:
            part[leg] = dict(stat(rate[leg], 1), unit="exposures/s")
        part["ratio_ima_over_none"] = round(part["device_complete_ima"]["median"] / part["device_complete"]["median"], 4)
        out["reads"][np.dtype(dtype).name] = part
        for slot in range(4):
            ctx.upload(slot, descs[slot])                      # (the option off again)

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
    print("wrote", out_path)


if __name__ == "__main__":
    main()
