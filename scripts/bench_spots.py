#!/usr/bin/env python3
"""Star spots (wayne_exposure_set_spots, k_lightcurve_spots): the rule's error, and the kernel's cost on the metric's
configuration (cfg4: K = 128 sub-samples, W = 4494 bins) -- not part of bench.py.

    python scripts/bench_spots.py [cfg4] [exposures per pass] [passes] > profiles/spots.json
    python scripts/bench_spots.py --rule-only > profiles/spots.json          (no GPU)

"rule": the worst |Q_n - Q_n(48 nodes)| / lens area of the 10-node rule over spots.rule_check_lenses(seed 1, 300 lenses);
tests/test_spots.py bounds the rule by 4 x this value.  CPU arithmetic.

"exposures" (GPU): in one process, for a mid-transit exposure of the synthetic visit,
  * clean: no spots (the light-curve launch alone);
  * no_crossing: one spot away from the planet's track (the rescale alone: d >= p + r is decided before any node);
  * one_crossing: one spot under the track (every wavelength of the crossing sub-samples evaluates 200 nodes);
  * eight_spots: eight spots, one of them under the track;
the k_lightcurve_spots launch and the light-curve launch by HIP events (profile slots "k_lightcurve_spots" and
"k_lightcurve"), median of `passes` passes of `exposures` runs each, and device-complete exposures/s: the same
descriptor uploaded into four slots in rotation and run, n exposures between two synchronisations, median of `passes`.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wayne_amd import spots  # noqa: E402


def rule_record():
    lenses = spots.rule_check_lenses(seed=1, n=300)
    return {"seed": 1, "lenses": len(lenses), "nodes": spots.GL_NODES, "converged_nodes": 48,
            "worst_error_over_area": spots.rule_error(lenses, 48)}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = {"rule": rule_record()}
    print("rule: worst |Q_n - Q_n(48)| / area = %.3e" % out["rule"]["worst_error_over_area"], file=sys.stderr, flush=True)
    if "--rule-only" in sys.argv:
        print(json.dumps(out, indent=1, sort_keys=True))
        return
    from wayne_amd import _lib, calibration, detector, engine, grism, synthetic, tools
    from wayne_amd.exposure_generator import ExposureGenerator
    name = args[0] if len(args) > 0 else "cfg4"
    n = int(args[1]) if len(args) > 1 else 100
    passes = int(args[2]) if len(args) > 2 else 5
    cal = calibration.CalibrationSet.synthetic(11)
    det = detector.WFC3_IR()
    gr = grism.G141(cal)
    v = synthetic.Visit(name, det, gr, cal, n_exposures=1)
    eng = engine.get_engine(0, gr, det, cal, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)
    ctx = eng.ctx
    i0, i1 = tools.crop_spectrum_ind(gr.wl_limits[0], gr.wl_limits[1], v.wl)
    mid = 0.5 * float(v.read_times[-1]) / 86400.0
    v.exp_start_days = np.array([-mid])                 # mid-transit at mid-exposure
    v.spots = None
    track = v.device_depths(0)
    from wayne_amd import lightcurve
    t = v.exp_start_days[0] + v.sample_mid_points / 86400e3
    _, _, X, Y = lightcurve.depth_inputs_track(mid_time=0.0, time_array=t, rp_white=np.sqrt(v.depth0.mean()), **v.ORBIT)
    xm, ym = float(X[len(X) // 2]), float(Y[len(Y) // 2])
    away = [(-0.5, 0.3, 0.1, 0.7)]
    under = [(xm, ym, 0.1, 0.7)]
    assert ym < -0.3                                    # (the synthetic orbit passes below the centre)
    others = [(-0.5, 0.3, 0.1, 0.6), (0.5, 0.3, 0.08, 1.1), (0.0, 0.7, 0.1, 0.8), (-0.7, 0.1, 0.05, 0.5),
              (0.7, 0.1, 0.05, 0.9), (0.0, 0.2, 0.1, 0.75), (-0.3, 0.75, 0.07, 0.65)]
    cases = {"clean": None, "no_crossing": away, "one_crossing": under, "eight_spots": under + others}
    out.update({"config": name, "sub_samples": int(v.K), "wavelength_bins": int(i1 - i0), "exposures_per_pass": n,
                "passes": passes, "library": os.path.relpath(_lib.library_info()[0], ROOT), "exposures": {},
                "planet_at_mid_exposure": [xm, ym], "z_range": [float(track.z_tr.min()), float(track.z_tr.max())]})
    for label, lst in cases.items():
        v.spots = None if lst is None else spots.StarSpots([spots.Spot(x, y, r, contrast=c) for (x, y, r, c) in lst])
        dd = v.device_depths(0)
        eg = ExposureGenerator(det, gr, v.NSAMP, v.SAMPSEQ, v.SUBARRAY, calibration=cal, seed=v.seed)
        desc = eg.build_descriptor(eng, rng_mode=_lib.RNG_SPLIT, out_dtype=np.float32, **v.frame_kwargs(0, planet_signal=dd))
        assert (desc._spots is not None) == (lst is not None)
        rec = {"spots": 0 if lst is None else len(lst)}
        if lst is not None:
            p_max = float(np.sqrt(dd.planet_spectrum[i0:i1].max()))
            rec["crossing_sub_sample_spot_pairs"] = int(sum(
                (np.hypot(dd.spots.X - x, dd.spots.Y - y) < p_max + r).sum() for (x, y, r, c) in lst))
        ctx.profile_enable(True)
        ctx.profile_select(["k_lightcurve", "k_lightcurve_spots"])
        us_lc, us_sp = [], []
        for rep in range(passes + 1):                  # (the first pass warms up)
            ctx.profile_reset()
            for i in range(n):
                ctx.upload(0, desc)
                ctx.run(0)
            ctx.synchronize()
            p = ctx.profile_get()["k_lightcurve"]
            launches, ms = ctx.spots_profile()
            assert p["launches"] == n and launches == (n if lst is not None else 0)
            if rep:
                us_lc.append(p["ms"] / n * 1e3)
                us_sp.append(ms / n * 1e3)
        ctx.profile_enable(False)
        ctx.profile_select(None)
        rate = []
        for rep in range(passes + 1):
            ctx.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                ctx.upload(i % 4, desc)
                ctx.run(i % 4)
            ctx.synchronize()
            if rep:
                rate.append(n / (time.perf_counter() - t0))
        rec.update({"lightcurve_launch_us": round(float(np.median(us_lc)), 2),
                    "spots_launch_us": round(float(np.median(us_sp)), 2),
                    "spots_launch_us_passes": [round(x, 2) for x in us_sp],
                    "device_complete_exposures_per_s": round(float(np.median(rate)), 1),
                    "device_complete_passes": [round(x, 1) for x in rate]})
        print("%-13s light-curve launch %7.2f us   spots launch %8.2f us   %7.1f exposures/s" % (
            label, rec["lightcurve_launch_us"], rec["spots_launch_us"], rec["device_complete_exposures_per_s"]),
            file=sys.stderr, flush=True)
        out["exposures"][label] = rec
    engine.close_all()                                 # (the context goes before the interpreter's teardown)
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
