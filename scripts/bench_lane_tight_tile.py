#!/usr/bin/env python3
"""k_lane with its test-free tiles sized for the refined radius, 6.9 sigma (knob lane_tight_tile = 0) against tiles sized
for the 16-bit radius, kLaneR16 = 4.63 sigma (lane_tight_tile = 1, the default), side by side in one process -- GPU
only; not part of bench.py.

    python scripts/bench_lane_tight_tile.py [cfg4] [exposures per pass] [repeats] [--out FILE]

Per setting: the kernel's own time (HIP events around every k_lane launch of 48 exposures) and the device-complete
exposures/s of resident descriptors on one stream, each the median of `repeats` passes with their spread (max - min),
the two settings taking turns pass by pass so that a drift of the box falls on both (the pattern of
scripts/bench_narrow_compact.py).  The sha256 of the reads of two exposures of cfg4, cfg3, cfg2 and cfg1 is taken under
both settings: the knob changes no frame.  And the share of k_lane's workgroups whose tile is test-free under either
rule, from a numpy restatement of the tile rule (k_narrow.h, lane_body) on the positions the device worked out
(wayne_exposure_debug_fetch); a bin counts as populated when it received electrons at all -- on these configurations
every such bin has wide electrons for its lane.
"""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wayne_amd import calibration, detector, engine, grism, synthetic, tools, visit as wvisit  # noqa: E402

SETTINGS = (("r34", 0), ("r16", 1))
REACH = {"r34": 6.9, "r16": 4.63}
LANE_THREADS, LANE_TILE, LANE_REACH_MAX = 512, 9216, 48


def stat(vals, digits=2):
    return {"median": round(float(np.median(vals)), digits), "spread": round(float(max(vals) - min(vals)), digits),
            "repetitions": [round(float(x), digits) for x in vals]}


def test_free_share(counts, x, y, sig_h, sig_l, N, reach):
    """Share of the (sub-sample, chunk of 512 bins) workgroups with electrons whose tile is test-free, and the mean
    tile area of those that are."""
    K, W = counts.shape
    free, busy, cells = 0, 0, 0
    smax = np.maximum(sig_h, sig_l).astype(np.float32)
    for k in range(K):
        for lo in range(0, W, LANE_THREADS):
            s = slice(lo, lo + LANE_THREADS)
            m = counts[k, s] > 0
            if not m.any():
                continue
            busy += 1
            r = np.float32(reach) * smax[s][m].max() + np.float32(1.0)
            if not r <= LANE_REACH_MAX:
                continue
            mg = int(np.ceil(r))
            ix, iy = np.floor(x[k, s][m]).astype(np.int64), np.floor(y[k, s][m]).astype(np.int64)
            x0, x1, y0, y1 = ix.min() - mg, ix.max() + mg + 1, iy.min() - mg, iy.max() + mg + 1
            area = (x1 - x0) * (y1 - y0)
            if x0 >= 1 and y0 >= 1 and x1 <= N and y1 <= N and area <= LANE_TILE:
                free += 1
                cells += area
    return {"workgroups": busy, "test_free": free, "share": round(free / max(busy, 1), 4),
            "mean_test_free_tile_cells": round(cells / max(free, 1), 1)}


def setup(name):
    cal = calibration.CalibrationSet.synthetic(11)
    det, gr = detector.WFC3_IR(), grism.G141(cal)
    v = synthetic.Visit(name, det, gr, cal, n_exposures=8)
    runner = wvisit.VisitRunner(v, 0, out_dtype=np.float32)
    eng = runner.engine()
    eng.ctx.set_knob("streams", 1)
    eng.ctx.set_knob("fuse_thrower", 0)                    # k_lane as a launch of its own (not inside k_thrower)
    for slot in range(4):
        eng.ctx.upload(slot, runner.descriptor(slot, eng))
    eng.ctx.synchronize()
    return v, gr, eng.ctx


def reads_sha(ctx):
    """sha256 of the reads of two exposures under both settings."""
    sha = {}
    for label, knob in SETTINGS:
        ctx.set_knob("lane_tight_tile", knob)
        h = hashlib.sha256()
        for slot in (0, 3):
            ctx.run(slot)
            ctx.synchronize()
            h.update(np.ascontiguousarray(ctx.download(slot)).tobytes())
        sha[label] = h.hexdigest()[:32]
    return sha


def main():
    argv = list(sys.argv[1:])
    out_path = None
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
        del argv[argv.index("--out"):argv.index("--out") + 2]
    name = argv[0] if len(argv) > 0 else "cfg4"
    n = int(argv[1]) if len(argv) > 1 else 200
    repeats = int(argv[2]) if len(argv) > 2 else 5

    v, gr, ctx = setup(name)
    out = {"config": name, "exposures_per_pass": n, "repeats": repeats, "streams": 1}
    rate = {label: [] for label, _ in SETTINGS}
    lane_us = {label: [] for label, _ in SETTINGS}
    for rep in range(repeats + 1):                         # (the first pass warms up)
        for label, knob in SETTINGS:
            ctx.set_knob("lane_tight_tile", knob)
            for j in range(8):
                ctx.run(j % 4)
            ctx.synchronize()
            t0 = time.perf_counter()
            for j in range(n):
                ctx.run(j % 4)
            ctx.synchronize()
            dc = n / (time.perf_counter() - t0)
            ctx.profile_enable(True)
            ctx.profile_select(["k_lane"])
            ctx.profile_reset()
            for j in range(48):
                ctx.run(j % 4)
            ctx.synchronize()
            p = ctx.profile_get()["k_lane"]
            ctx.profile_enable(False)
            ctx.profile_select(None)
            if rep > 0:
                rate[label].append(dc)
                lane_us[label].append(p["ms"] / max(p["launches"], 1) * 1e3)
    out["k_lane_us"] = {label: stat(lane_us[label]) for label, _ in SETTINGS}
    out["device_complete"] = {label: dict(stat(rate[label], 1), unit="exposures/s") for label, _ in SETTINGS}

    # the tile rule restated on the device's own positions
    counts, x, y, _ = ctx.debug_fetch(0)
    i0, i1 = tools.crop_spectrum_ind(gr.wl_limits[0], gr.wl_limits[-1], v.wl.copy())
    wl = v.wl[i0:i1]
    assert wl.size == counts.shape[1], (wl.size, counts.shape)
    sig_h, sig_l = gr.psf_sigmah_poly(wl), gr.psf_sigmal_poly(wl)
    N = 1014 if v.SUBARRAY == 1024 else v.SUBARRAY      # (the frame without its reference-pixel border)
    out["sigma_h_px"] = [round(float(sig_h.min()), 3), round(float(sig_h.max()), 3)]
    out["test_free"] = {label: test_free_share(counts, x, y, sig_h, sig_l, N, REACH[label]) for label, _ in SETTINGS}

    sha = {name: reads_sha(ctx)}
    engine.close_all()
    for other in ("cfg3", "cfg2", "cfg1"):
        if other != name:
            sha[other] = reads_sha(setup(other)[2])
            engine.close_all()
    out["reads_sha256_slots_0_3"] = sha
    out["reads_identical"] = all(s["r34"] == s["r16"] for s in sha.values())
    text = json.dumps(out, indent=1)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
