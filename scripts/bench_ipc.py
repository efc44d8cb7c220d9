#!/usr/bin/env python3
"""The cost of inter-pixel capacitance (k_ipc and k_ipc_clear) beside an exposure, on the metric's configuration: the
two kernels' HIP-event time (one interval spans both: wayne_ipc_profile; exposures on one stream), the live fraction they worked on -- the (wave,
read interval) pairs whose 64 accumulators meet the interval's dilated box, of all pairs -- the bytes that work has to
move against 8 TB/s, and device-complete exposures per second with and without the option over four resident slots on
the context's two streams.  Both legs in one process, medians of `repeats` passes behind a warm-up pass.  GPU only.  No
test asserts any of it.

    python scripts/bench_ipc.py [config=cfg4] [exposures per pass=200] [repeats=5] [--out profiles/ipc.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wayne_amd import _lib, calibration, detector, grism, ipc, synthetic, visit as wvisit  # noqa: E402

HBM_BYTES_PER_S = 8e12


def stat(vals, digits=2):
    return {"median": round(float(np.median(vals)), digits), "spread": round(float(max(vals) - min(vals)), digits),
            "repetitions": [round(float(x), digits) for x in vals]}


def live_pairs(boxes, R, S, dilate):
    """(wave, read interval) pairs k_ramp's box test calls live (wayne_exposure_debug_boxes states it), the boxes dilated
    by `dilate` pixels and clamped to the frame.  Cosmic-ray segments come on top: a few dozen waves an exposure."""
    n = S * S
    p0 = np.arange(0, n, 64)
    wy0, wy1 = p0 // S, np.minimum(p0 + 63, n - 1) // S
    wx0 = p0 - wy0 * S
    live = 0
    for r in range(R):
        x0, x1, y0, y1 = (int(v) for v in boxes[r])
        if x0 >= x1 or y0 >= y1:
            continue
        x0, x1, y0, y1 = max(x0 - dilate, 0), min(x1 + dilate, S), max(y0 - dilate, 0), min(y1 + dilate, S)
        rows = (wy0 < y1) & (wy1 >= y0)
        cols = (wy0 != wy1) | ((wx0 < x1) & (wx0 + 64 > x0))
        live += int((rows & cols).sum())
    return live, R * len(p0)


def main():
    argv = list(sys.argv[1:])
    out_path = os.path.join(ROOT, "profiles", "ipc.json")
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
    S, R = ctx.S, v.NSAMP - 1
    model = ipc.InterpixelCapacitance()
    descs = [runner.generator(i).build_descriptor(eng, out_dtype=np.float32, rng_mode=runner.rng_mode, **runner.frame_kwargs(i))
             for i in range(4)]

    def make_resident(opt):
        for slot in range(4):
            ctx.upload(slot, descs[slot])
            if opt is not None:
                ctx.set_ipc(slot, opt)

    def device_complete(count):
        t0 = time.perf_counter()
        for j in range(count):
            ctx.run(j % 4)
        ctx.synchronize()
        return count / (time.perf_counter() - t0)

    legs = ("device_complete", "device_complete_ipc")
    rate = {leg: [] for leg in legs}
    kernel_us = []
    for rep in range(repeats + 1):                         # (the first pass warms up: allocations, code objects)
        got = {}
        make_resident(None)
        device_complete(8)
        got["device_complete"] = device_complete(n)
        make_resident(model)
        device_complete(8)
        got["device_complete_ipc"] = device_complete(n)
        # the kernels alone: HIP events around their two launches
        ctx.profile_enable(True)
        ctx.profile_select(["k_ipc"])
        ctx.profile_reset()
        for j in range(min(n, 48)):
            ctx.run((j % 2) * 2)                           # (one stream: nothing else runs inside the interval)
        ctx.synchronize()
        launches, ms = ctx.ipc_profile()
        ctx.profile_enable(False)
        ctx.profile_select(None)
        if rep > 0:
            for leg in legs:
                rate[leg].append(got[leg])
            kernel_us.append(ms / max(launches, 1) * 1e3)

    make_resident(None)                                    # (the option off again: debug_boxes then reports the planner's own boxes)
    use_box, boxes, _ = ctx.debug_boxes(0)
    live_d, pairs = live_pairs(boxes, R, S, 1) if use_box else (R * ((S * S + 63) // 64),) * 2
    live_0, _ = live_pairs(boxes, R, S, 0) if use_box else (live_d, pairs)
    # k_ipc reads each live accumulator once from HBM (its eight neighbours come from the cache) and writes one; k_ipc_clear
    # writes one per accumulator of the undilated set
    moved = live_d * 64 * 16 + live_0 * 64 * 8
    us = float(np.median(kernel_us))
    out = {"config": name, "S": S, "NSAMP": v.NSAMP, "exposures_per_pass": n, "repeats": repeats,
           "library": _lib.library_info()[0].replace(ROOT + os.sep, ""), "kernel": model.kernel.tolist(),
           "weights": model.weights().tolist(), "ramp_variant": ctx.ramp_variant(0), "use_box": bool(use_box),
           "k_ipc_and_clear_us": stat(kernel_us, 1),
           "live": {"pairs": pairs, "dilated": live_d, "undilated": live_0, "fraction": round(live_d / pairs, 4)},
           "bytes_moved": {"total": moved, "us_at_8_TB_per_s": round(moved / HBM_BYTES_PER_S * 1e6, 2),
                           "bytes_per_s": moved / (us * 1e-6) if us > 0 else None,
                           "fraction_of_8_TB_per_s": round(moved / (us * 1e-6) / HBM_BYTES_PER_S, 4) if us > 0 else None}}
    for leg in legs:
        out[leg] = dict(stat(rate[leg], 1), unit="exposures/s")
    out["ratio_ipc_over_none"] = round(out["device_complete_ipc"]["median"] / out["device_complete"]["median"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
    print("wrote", out_path)


if __name__ == "__main__":
    main()
