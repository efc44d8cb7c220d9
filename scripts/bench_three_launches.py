#!/usr/bin/env python3
"""The launch sequence of an exposure, five launches against three, side by side in one process -- GPU only; not part of
bench.py.  Two knobs, four combinations:

    prep_wl_per_run  1: k_prep_wl_run in front of every run (per-wavelength arrays, trace coefficients, status clear), as
                        it was; 0 (the default): nothing in front of k_prep_sub
    fuse_thrower     0: k_lane and k_narrow as two launches, as it was; 1 (the default): one grid for both, k_thrower

    python scripts/bench_three_launches.py [cfg4] [exposures per pass] [repeats] [--out FILE]

Per combination: the thrower's time by HIP events (the PK_THROW interval + k_narrow's own, which is how bench.py adds
them up, over 48 exposures) and the device-complete exposures/s of resident descriptors on one stream, each the median
of `repeats` passes with their spread (max - min), the combinations taking turns pass by pass so that a drift of the box
falls on all of them (the pattern of scripts/bench_narrow_compact.py).  The sha256 of the last exposure's reads is taken
under every combination: the knobs change no frame.
"""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wayne_amd import calibration, detector, engine, grism, synthetic, visit as wvisit  # noqa: E402

SETTINGS = (("prep_per_run+two_launches", (1, 0)), ("prep_per_run+one_grid", (1, 1)),
            ("prep_at_upload+two_launches", (0, 0)), ("prep_at_upload+one_grid", (0, 1)))


def stat(vals, digits=2):
    return {"median": round(float(np.median(vals)), digits), "spread": round(float(max(vals) - min(vals)), digits),
            "repetitions": [round(float(x), digits) for x in vals]}


def main():
    argv = list(sys.argv[1:])
    out_path = None
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
        del argv[argv.index("--out"):argv.index("--out") + 2]
    name = argv[0] if len(argv) > 0 else "cfg4"
    n = int(argv[1]) if len(argv) > 1 else 200
    repeats = int(argv[2]) if len(argv) > 2 else 5

    cal = calibration.CalibrationSet.synthetic(11)
    det, gr = detector.WFC3_IR(), grism.G141(cal)
    v = synthetic.Visit(name, det, gr, cal, n_exposures=8)
    runner = wvisit.VisitRunner(v, 0, out_dtype=np.float32)
    eng = runner.engine()
    ctx = eng.ctx
    ctx.set_knob("streams", 1)
    for slot in range(4):
        ctx.upload(slot, runner.descriptor(slot, eng))
    ctx.synchronize()

    out = {"config": name, "exposures_per_pass": n, "repeats": repeats, "streams": 1}
    rate = {label: [] for label, _ in SETTINGS}
    thrower_us = {label: [] for label, _ in SETTINGS}
    launches = {}
    sha = {}
    for rep in range(repeats + 1):                         # (the first pass warms up)
        for label, knob in SETTINGS:
            ctx.set_knob("prep_wl_per_run", knob[0])
            ctx.set_knob("fuse_thrower", knob[1])
            for j in range(8):
                ctx.run(j % 4)
            ctx.synchronize()
            t0 = time.perf_counter()
            for j in range(n):
                ctx.run(j % 4)
            ctx.synchronize()
            dc = n / (time.perf_counter() - t0)
            ctx.profile_enable(True)
            ctx.profile_select(["k_prep_wl", "k_throw", "k_narrow"])
            ctx.profile_reset()
            for j in range(48):
                ctx.run(j % 4)
            ctx.synchronize()
            p = ctx.profile_get()
            ctx.profile_enable(False)
            ctx.profile_select(None)
            if rep > 0:
                rate[label].append(dc)
                thrower_us[label].append((p["k_throw"]["ms"] + p["k_narrow"]["ms"]) / 48 * 1e3)
            if rep == repeats:
                launches[label] = {"k_prep_wl": p["k_prep_wl"]["launches"] // 48, "k_throw_intervals": p["k_throw"]["launches"] // 48,
                                   "k_narrow": p["k_narrow"]["launches"] // 48}
                sha[label] = hashlib.sha256(np.ascontiguousarray(ctx.download(3)).tobytes()).hexdigest()[:32]
    out["thrower_us"] = {label: stat(thrower_us[label]) for label, _ in SETTINGS}
    out["device_complete"] = {label: dict(stat(rate[label], 1), unit="exposures/s") for label, _ in SETTINGS}
    out["intervals_per_exposure"] = launches
    out["reads_sha256_slot3"] = sha
    out["reads_identical"] = len(set(sha.values())) == 1
    engine.close_all()
    text = json.dumps(out, indent=1)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
