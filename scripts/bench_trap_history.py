#!/usr/bin/env python3
"""Cost of a carried trap history (wayne_exposure_set_trap_history, k_ramp_hist) beside planned start tables
(k_ramp_trap), and what the planned shortcut costs a light curve -- GPU only; not part of bench.py.

    python scripts/bench_trap_history.py [cfg4] [exposures per pass] [passes] [out.json]

Rates: the same descriptor uploaded into slots 0 .. 3 in rotation and run, n exposures between two synchronisations
(device-complete), and the same loop with every exposure's reads fetched to pinned host memory, two in flight
(delivered); all legs in one process, the median of `passes` passes after one that warms up.  Legs:
    planned            start tables, k_ramp_trap (today's path)
    planned_general    ... with knob throw_wgs = 1024: the general launch sequence a carried slot always takes (k_throw
                       launched although it finds nothing to do), without the state
    carried            the trap state carried, k_ramp_hist
    planned_1stream / carried_1stream: knob streams = 1, where the serialised ramp kernels cost no overlap
    planned_again      the first leg once more, last: what the order of the legs does to a rate
and the ramp kernel's own time (HIP events, one exposure at a time) for planned and carried.
The motivating figure: the mini visit of tests/fixtures in both modes, per exposure the white-light difference
(carried - planned) / planned of the last read minus the zero read, in ppm.
Writes profiles/trap_history.json (or the path given).
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wayne_amd import _lib, calibration, detector, engine, grism, run_visit, synthetic, traps  # noqa: E402
from wayne_amd.exposure_generator import ExposureGenerator  # noqa: E402


def rates(ctx, desc, tr, n, passes, delivered):
    """Median exposures/s over `passes` passes of n exposures."""
    got = []
    for rep in range(passes + 1):
        if isinstance(tr, traps.CarriedTraps):
            ctx.trap_state_reset(tr.traps.array("initial"))
        ctx.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            slot = i % 4
            if delivered and i >= 2:
                ctx.wait((i - 2) % 4)
            ctx.upload(slot, desc)
            ctx.set_traps(slot, tr)
            if isinstance(tr, traps.CarriedTraps):
                ctx.set_trap_history(slot, tr)
            ctx.run(slot)
            if delivered:
                ctx.fetch_async(slot)
        if delivered:
            for i in range(max(n - 2, 0), n):
                ctx.wait(i % 4)
        ctx.synchronize()
        if rep > 0:
            got.append(n / (time.perf_counter() - t0))
    return round(statistics.median(got), 1), [round(g, 1) for g in got]


def ramp_kernel_us(ctx, desc, tr, n):
    ctx.profile_enable(True)
    ctx.profile_select(["k_ramp"])
    ctx.profile_reset()
    for i in range(n):
        ctx.upload(0, desc)
        ctx.set_traps(0, tr)
        if isinstance(tr, traps.CarriedTraps):
            ctx.set_trap_history(0, tr)
        ctx.run(0)
    p = ctx.profile_get()["k_ramp"]
    ctx.profile_enable(False)
    ctx.profile_select(None)
    return round(p["ms"] / max(p["launches"], 1) * 1e3, 2)


def white_light_ppm():
    """Per exposure of the mini visit: (carried - planned) / planned of the frame's summed last read minus zero read, ppm."""
    import yaml
    mini = os.path.join(ROOT, "tests", "fixtures", "mini_visit")
    white = {}
    for mode in ("planned", "carried"):
        cfg = yaml.safe_load(open(os.path.join(mini, "params.yml")))
        cfg["charge_traps"] = {"history": mode}
        obs = run_visit.build_observation(cfg, base_dir=mini)
        obs.frame_options["out_dtype"] = np.float64
        frames = obs.run_observation(write_fits=False)
        n = len(obs.exp_start_times)
        white[mode] = np.array([float((np.asarray(frames[i + 1].reads[-1][0], dtype=np.float64)
                                       - np.asarray(frames[i + 1].reads[0][0], dtype=np.float64)).sum()) for i in range(n)])
    return [round(float(v), 2) for v in (white["carried"] - white["planned"]) / white["planned"] * 1e6]


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "cfg4"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    passes = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "trap_history.json")
    cal = calibration.CalibrationSet.synthetic(11)
    det = detector.WFC3_IR()
    gr = grism.G141(cal)
    v = synthetic.Visit(name, det, gr, cal, n_exposures=1)
    eng = engine.get_engine(0, gr, det, cal, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)
    ctx = eng.ctx
    eg = ExposureGenerator(det, gr, v.NSAMP, v.SAMPSEQ, v.SUBARRAY, calibration=cal, seed=v.seed)
    desc = eg.build_descriptor(eng, rng_mode=_lib.RNG_SPLIT, out_dtype=np.float32, **v.frame_kwargs(0))
    model = traps.ChargeTraps()
    exptime = float(v.read_times[-1])
    t = [o * 96.0 / 1440.0 + k * (exptime + 60.0) / 86400.0 for o in range(2) for k in range(4)]
    plan = {"exp_start_times": np.array(t), "orbit_start_index": [0, 4]}
    planned = traps.ExposureTraps(model, model.start_tables(plan, exptime, staring=False)[5])
    carried = model.carried(model.history_plan(plan, exptime, staring=False), 5)

    out = {"config": name, "exposures_per_pass": n, "passes": passes, "state_bytes_per_exposure": 16 * ctx.S * ctx.S,
           "device_complete_per_s": {}, "delivered_per_s": {}, "passes_per_s": {}, "ramp_kernel_us": {}, "variant": {}}
    legs = [("planned", planned, {}), ("planned_general", planned, {"throw_wgs": 1024}), ("carried", carried, {}),
            ("planned_1stream", planned, {"streams": 1}), ("carried_1stream", carried, {"streams": 1}),
            ("planned_again", planned, {})]
    for label, tr, knobs in legs:
        for k, val in knobs.items():
            ctx.set_knob(k, val)
        try:
            dc, dc_all = rates(ctx, desc, tr, n, passes, delivered=False)
            dl, dl_all = rates(ctx, desc, tr, n, passes, delivered=True)
        finally:
            for k in knobs:
                ctx.set_knob(k, None)
        out["device_complete_per_s"][label], out["delivered_per_s"][label] = dc, dl
        out["passes_per_s"][label] = {"device_complete": dc_all, "delivered": dl_all}
        out["variant"][label] = ctx.ramp_variant(0)
        print("%-16s device-complete %8.1f /s   delivered %8.1f /s   %s" % (label, dc, dl, out["variant"][label]), flush=True)
    ctx.trap_state_reset(model.array("initial"))
    for label, tr in (("planned", planned), ("carried", carried)):
        out["ramp_kernel_us"][label] = ramp_kernel_us(ctx, desc, tr, min(n, 100))
    print("ramp kernel us:", out["ramp_kernel_us"], flush=True)
    out["mini_visit_white_light_ppm_carried_minus_planned"] = white_light_ppm()
    print("white light, carried - planned (ppm):", out["mini_visit_white_light_ppm_carried_minus_planned"], flush=True)
    engine.close_all()
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
