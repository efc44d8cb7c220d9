#!/usr/bin/env python3
"""k_narrow with its pooled row chains on their groups' lanes (knob narrow_compact = 0) against the chains compacted
across the workgroup (narrow_compact = 1, the default), side by side in one process -- GPU only; not part of bench.py.

    python scripts/bench_narrow_compact.py [cfg4] [exposures per pass] [repeats] [--out FILE]

Per setting: the kernel's own time (HIP events around every k_narrow launch of 48 exposures) and the device-complete
exposures/s of resident descriptors on one stream, each the median of `repeats` passes with their spread (max - min),
the two settings taking turns pass by pass so that a drift of the box falls on both (the pattern of
scripts/bench_u16_reads.py).  The sha256 of the last exposure's reads is taken under both settings: the knob changes
no frame.
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

SETTINGS = (("per_group", 0), ("compact", 1))


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
    narrow_us = {label: [] for label, _ in SETTINGS}
    sha = {}
    for rep in range(repeats + 1):                         # (the first pass warms up)
        for label, knob in SETTINGS:
            ctx.set_knob("narrow_compact", knob)
            for j in range(8):
                ctx.run(j % 4)
            ctx.synchronize()
            t0 = time.perf_counter()
            for j in range(n):
                ctx.run(j % 4)
            ctx.synchronize()
            dc = n / (time.perf_counter() - t0)
            ctx.profile_enable(True)
            ctx.profile_select(["k_narrow"])
            ctx.profile_reset()
            for j in range(48):
                ctx.run(j % 4)
            ctx.synchronize()
            p = ctx.profile_get()["k_narrow"]
            ctx.profile_enable(False)
            ctx.profile_select(None)
            if rep > 0:
                rate[label].append(dc)
                narrow_us[label].append(p["ms"] / max(p["launches"], 1) * 1e3)
            if rep == repeats:
                sha[label] = hashlib.sha256(np.ascontiguousarray(ctx.download(3)).tobytes()).hexdigest()[:32]
    out["k_narrow_us"] = {label: stat(narrow_us[label]) for label, _ in SETTINGS}
    out["device_complete"] = {label: dict(stat(rate[label], 1), unit="exposures/s") for label, _ in SETTINGS}
    out["reads_sha256_slot3"] = sha
    out["reads_identical"] = sha["per_group"] == sha["compact"]
    engine.close_all()
    text = json.dumps(out, indent=1)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
